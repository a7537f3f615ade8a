"""greedy decoding speed at Vicuna-7B (or --13b, optionally --fp8; --small: config.gpt2_small_shaped()), B=8: prefill of a ~600-token
prompt, then N single-token steps through the K/V cache -- host loop (token choice on the host, one sync per token) vs device loop
(eager) vs device loop replayed from a hipGraph (navillm_amd/kvcache.py).
--trie[=WORDS,DEPTH] (default 2000,24): the same three loops under a trie constraint -- WORDS random words of DEPTH tokens each, about
half of them branching off an earlier word, so every row decodes DEPTH tokens and then eos.  --reps=R timed calls per loop (default 2;
the last one is reported, with the spread over all but the first); --free with --trie: the unconstrained loops as well.
--sample [--temperature=T --top-k=K --top-p=P] (defaults 0.01, 50 and none: the reference's evaluation scripts run --do_sample
--temperature 0.01): generate(do_sample=True) instead, host loop (torch topk / softmax / multinomial per token) vs the device loop of
NAVILLM_DEVICE_SAMPLE; --top-p adds the nucleus warper to both (without it the call carries no top_p at all); combines with --trie,
--small and --free.
--rep-penalty=P and --min-new=N: generate(repetition_penalty=P, min_new_tokens=N) in every loop measured (--min-new not with --trie);
without them the call carries neither keyword."""
import sys, os, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navillm_amd import config as nvcfg
import navillm_amd.kvcache as kvm
from navillm_amd.nav_model import NavModel
from navillm_amd.kvcache import KVCacheLM


def opt(name, default):
    return next((a.split('=', 1)[1] for a in sys.argv if a.startswith(f'--{name}=')), default)


class Node:
    def __init__(self):
        self.child = {}


class Trie:
    """tools/trie.py protocol of the reference (root / get_child_index / get_next_node)"""
    def __init__(self, words, eos):
        self.root, self.eos = Node(), eos
        for w in words:
            cur = self.root
            for c in w:
                cur = cur.child.setdefault(c, Node())

    def get_child_index(self, cur):
        return [self.eos] if not cur.child else list(cur.child.keys())

    def get_next_node(self, cur, w):
        return cur.child[w] if w in cur.child else cur


def random_trie(n_words, depth, vocab, eos, g):
    words = []
    for _ in range(n_words):
        w = torch.randint(3, vocab, (depth,), generator=g).tolist()
        if words and float(torch.rand((), generator=g)) < 0.5:
            k = int(torch.randint(1, depth, (), generator=g))
            w = words[int(torch.randint(len(words), (), generator=g))][:k] + w[k:]
        words.append(w)
    return Trie(words, eos)


dev = torch.device("cuda:0")
small = "--small" in sys.argv
cfg = nvcfg.gpt2_small_shaped() if small else nvcfg.vicuna_13b() if "--13b" in sys.argv else nvcfg.vicuna_7b()
model = NavModel(nav_config=cfg, device=dev, seed=0)
model.eval()
if "--fp8" in sys.argv:
    model.to_fp8_weight_only()
B = int(opt("batch", 8))
reps = int(opt("reps", 2))
L, N = int(opt("prompt", 600)), 64
g = torch.Generator().manual_seed(0)
ids = [[1] + torch.randint(3, cfg.base_vocab_size, (L - 1 + b,), generator=g).tolist() for b in range(B)]
sample = None
if "--sample" in sys.argv:
    sample = dict(do_sample=True, temperature=float(opt("temperature", 0.01)), top_k=int(opt("top-k", 50)))
    if opt("top-p", None) is not None:
        sample["top_p"] = float(opt("top-p", None))
procs = {}
if opt("rep-penalty", None) is not None:
    procs["repetition_penalty"] = float(opt("rep-penalty", None))
if opt("min-new", None) is not None:
    procs["min_new_tokens"] = int(opt("min-new", None))
trie, eos = None, -1
if any(a == "--trie" or a.startswith("--trie=") for a in sys.argv):
    n_words, depth = (int(x) for x in opt("trie", "2000,24").split(","))
    eos = 2
    trie = random_trie(n_words, depth, cfg.base_vocab_size, eos, g)
    N = depth + 1
wbytes = 2 * cfg.num_layers * (4 * cfg.hidden_size ** 2 + 3 * cfg.hidden_size * cfg.intermediate_size) / (2 if "--fp8" in sys.argv else 1)
kv = KVCacheLM(model, B, capacity=1024)
kv.extend([list(x) for x in ids]); torch.cuda.synchronize()
t0 = time.perf_counter(); kv.reset(); kv.extend([list(x) for x in ids]); torch.cuda.synchronize(); tp = time.perf_counter() - t0
name = "gpt2-small-shaped" if small else "13b" if "--13b" in sys.argv else "7b"
print(f"{name}{' fp8' if '--fp8' in sys.argv else ''}{' trie' if trie is not None else ''}{f' sampled {sample}' if sample else ''}{f' {procs}' if procs else ''}: prefill {B}x~{L}: {tp*1e3:.1f} ms")


def measure(trie, eos, N):
    print(f"  {'trie-constrained' if trie is not None else 'unconstrained'}, {N} new tokens:")
    for tag, devloop, graph in (("host loop", False, False), ("device loop, eager", True, False), ("device loop, hipGraph", True, True)):
        kvm.DEVICE_GREEDY, kvm.DEVICE_SAMPLE, kvm.USE_HIP_GRAPH = devloop, devloop, graph
        pers = []
        for rep in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            kw = dict(sample or {}, **procs, **({} if trie is None else {"trie": trie}))
            out = kv.generate(ids, max_new_tokens=N, eos_token_id=eos, pad_token_id=0, **kw)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            pers.append((dt - tp) / len(out[0]))
        per, warm = pers[-1], pers[1:]
        ran = (getattr(kv, "last_generate", None) or {}).get("loop", "?")
        print(f"  {tag:<24}: {per*1e3:.3f} ms per step of {B} tokens -> {B/per:.0f} tokens/s  (decoder weights once per step = {wbytes/per/1e12:.2f} TB/s)"
              f"  [{len(out[0])} steps, ran the {ran} loop, spread over {len(warm)} warm calls {min(warm)*1e3:.3f}..{max(warm)*1e3:.3f} ms]")


if trie is None or "--free" in sys.argv:
    measure(None, -1, 64)
if trie is not None:
    measure(trie, eos, N)
