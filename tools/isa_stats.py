"""Per-kernel statistics of a hipcc --save-temps assembly file: registers, scratch, occupancy, instruction counts of interest.
Usage: isa_stats.py FILE.s [substring filter ...]
       isa_stats.py --compare OLD.s NEW.s     same kernel symbols; per kernel scratch not above OLD's, the same occupancy, the same
                                              counts, and in every basic block that holds a v_mfma the same multiset of opcodes;
                                              prints what differs (and the instruction totals outside those blocks), exit 1 if any"""
import re, sys
from collections import Counter

KEYS = ("v_mfma\w*", "v_cvt_pk_f32_fp8", "v_pk_mul_f32", "v_cvt_pk_bf16_f32", "v_cvt_scalef32_pk_bf16_fp8", "ds_read_b64", "ds_read_b128",
        "ds_read_b64_tr_b16", "buffer_load_dwordx4", "s_barrier", "scratch_\w+", "s_waitcnt vmcnt\(0\)")


def kernels(path):
    s = open(path).read()
    out = {}
    for f in re.split(r"\n(?=\t\.section\t\.text\.)", s):
        m = re.search(r"^(_Z\S+):\s", f, re.M)
        if not m:
            continue
        name = m.group(1)
        def g(key):
            r = re.search(r"\.set " + re.escape(name) + r"\." + key + r", (\d+)", s)
            return r.group(1) if r else "?"
        occ = re.search(r"^; Occupancy: (\d+)", f, re.M)
        out[name] = dict(body=f, vgpr=g("num_vgpr"), agpr=g("num_agpr"), scratch=g("private_seg_size"), occ=occ.group(1) if occ else "?",
                         cnt={k: len(re.findall(r"^\s+" + k + r"\b", f, re.M)) for k in KEYS})
    return out


def blocks(body):
    """opcode multisets of the basic blocks of a kernel: (blocks holding a v_mfma, instructions in the others)"""
    code = body[:body.index("\ts_endpgm")] if "\ts_endpgm" in body else body
    mf, rest, cur = [], 0, Counter()
    def close():
        nonlocal cur, rest
        if any(k.startswith("v_mfma") for k in cur):
            mf.append(cur)
        else:
            rest += sum(cur.values())
        cur = Counter()
    for line in code.split("\n"):
        if re.match(r"^\.LBB\d+_\d+:", line):
            close()
            continue
        m = re.match(r"^\t([a-z]\w+)", line)
        if not m:
            continue
        cur[m.group(1)] += 1
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            close()
    close()
    return Counter(tuple(sorted(b.items())) for b in mf), rest


def short(name):
    return re.sub(r"_ZN12_GLOBAL__N_1", "", name)[:110]


def compare(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    if set(a) != set(b):
        bad += 1
        print("kernel symbols differ: only old", sorted(set(a) - set(b)), "only new", sorted(set(b) - set(a)))
    for name in sorted(set(a) & set(b)):
        x, y, notes = a[name], b[name], []
        if int(y["scratch"]) > int(x["scratch"]):
            notes.append(f"SCRATCH {x['scratch']} -> {y['scratch']}")
        elif y["scratch"] != x["scratch"]:
            notes.append(f"(scratch {x['scratch']} -> {y['scratch']})")
        if x["occ"] != y["occ"]:
            notes.append(f"OCCUPANCY {x['occ']} -> {y['occ']}")
        for k in KEYS:
            if k.startswith(("scratch", "s_waitcnt")):
                continue
            if x["cnt"][k] != y["cnt"][k]:
                notes.append(f"COUNT {k} {x['cnt'][k]} -> {y['cnt'][k]}")
        (mx, rx), (my, ry) = blocks(x["body"]), blocks(y["body"])
        detail = []
        if mx != my:
            notes.append(f"MFMA BLOCKS differ: {sum((mx - my).values())} only old, {sum((my - mx).values())} only new (of {sum(mx.values())})")
            only_new = [Counter(dict(q)) for q in (my - mx).elements()]
            for q in (mx - my).elements():          # each unmatched old block against the nearest unmatched new one
                co = Counter(dict(q))
                if not only_new:
                    detail.append(f"    block of {sum(co.values())} instructions ({sum(v for k, v in co.items() if k.startswith('v_mfma'))} MFMA): gone")
                    continue
                cn = min(only_new, key=lambda c: sum(((co - c) + (c - co)).values()))
                only_new.remove(cn)
                detail.append(f"    block of {sum(co.values())} instructions ({sum(v for k, v in co.items() if k.startswith('v_mfma'))} MFMA): "
                              f"old has more {dict(co - cn)}, new has more {dict(cn - co)}")
        bad += any(n[0] != "(" for n in notes)
        print(short(name), f"vgpr {x['vgpr']}->{y['vgpr']} outside-mfma-blocks {rx}->{ry}", "; ".join(notes) if notes else "same")
        for d in detail:
            print(d)
    print("DIFFERENT" if bad else "all kernels: same symbols, scratch, occupancy, counts and MFMA blocks")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    filt = sys.argv[2:]
    for name, k in kernels(sys.argv[1]).items():
        if filt and not any(x in name for x in filt):
            continue
        print(short(name), "vgpr", k["vgpr"], "agpr", k["agpr"], "scratch", k["scratch"], "occupancy", k["occ"], {q: v for q, v in k["cnt"].items() if v})
