// Device-side bookkeeping of greedy decoding (reference: HF generate(do_sample=False) as called from
// models/nav_model.py:324-341,388-402 with the special-id logit mask of models/modified_lm.py:122-124).
//
// One decode step is ~360 dependent kernel launches; with the token choice on the host every step also pays a device->host
// sync, the python index bookkeeping and an upload.  Here the choice and the bookkeeping are two tiny kernels, so a whole step
// (lm_head -> pick -> advance -> embed -> 32 decoder layers) has frozen launch arguments and is replayed from a hipGraph
// (navillm_amd/kvcache.py); the host only polls the `fin` flags, a step or two behind.
// Sampled decoding (HF sample(): temperature, top-k, top-p, one draw per row) is the same step with decode_pick_sample_kernel as its pick.
// HF's repetition penalty and minimum length (PickProcs below; the rule is stated once) are the PROC = true
// instantiations of the same three pick kernels; PROC = false is the pick without them.
//
// state layout (int32, one buffer): tok[B] | fin[B] | len[B] | pos[B] | crow[B] | grow[B] | last[B] | dyn[2] | cnt[1] | overflow[1]
#include "nv_common.h"

namespace {

// ---- what the pick kernels share: the pick rule, the block reduction and HF's bookkeeping
constexpr int PICK_NONE = 0x7fffffff;                             // "no candidate yet"

// a candidate id is pickable when it lies inside the vocabulary and outside the special range (models/modified_lm.py:122-124)
__device__ __forceinline__ bool pick_allowed(int v, int V, int special0, int nspecial) {
    return v < V && !(v >= special0 && v < special0 + nspecial);
}
// (x, v) replaces (best, bi): the largest value wins, ties go to the smallest id (like torch.argmax on the CPU)
__device__ __forceinline__ bool pick_beats(float x, int v, float best, int bi) {
    return v != PICK_NONE && (bi == PICK_NONE || x > best || (x == best && v < bi));
}
// block reduction of NT threads (value desc, id asc): inside each wave, then thread 0 over the NT / 64 waves; the result is valid in
// thread 0 only.  PAYLOAD: a third word travels with the winner (the trie kernel's edge index).
template <int NT, bool PAYLOAD>
__device__ __forceinline__ void pick_reduce(float& best, int& bi, int& be) {
    __shared__ float sv[NT / 64];
    __shared__ int si[NT / 64];
    __shared__ int se[PAYLOAD ? NT / 64 : 1];
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float x = __shfl_xor(best, o, 64);
        const int j = __shfl_xor(bi, o, 64);
        const int e = PAYLOAD ? __shfl_xor(be, o, 64) : 0;
        if (pick_beats(x, j, best, bi)) { best = x; bi = j; be = e; }
    }
    if ((tid & 63) == 0) {
        sv[tid >> 6] = best;
        si[tid >> 6] = bi;
        if (PAYLOAD) se[tid >> 6] = be;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NT / 64; ++w) {
            if (pick_beats(sv[w], si[w], best, bi)) { best = sv[w]; bi = si[w]; be = PAYLOAD ? se[w] : 0; }
        }
    }
}
// HF's bookkeeping for sample b (thread 0): a finished row emits `pad`; a row finishes when it emits `eos`; tok[b] and out[cnt, b]
// (while cnt < max_steps) take the token.  Returns whether the row had finished BEFORE this step.
__device__ __forceinline__ bool pick_emit(int* __restrict__ state, int* __restrict__ out, int max_steps, int B, int b, int picked, int eos,
                                          int pad) {
    int* tok = state;
    int* fin = state + B;
    const int cnt = state[7 * B + 2];
    const bool was = fin[b] != 0;
    const int nxt = was ? pad : picked;
    if (!was && nxt == eos) fin[b] = 1;
    tok[b] = nxt;
    if (cnt < max_steps) out[(long)cnt * B + b] = nxt;
    return was;
}

// ---- the logits processors (HF's RepetitionPenaltyLogitsProcessor, then MinNewTokensLengthLogitsProcessor), applied after the special-id
// mask and in front of everything else a pick does; DESIGN.md §4 "Logits processors" states the rule.
//   seen [B, seen_ld] (nullable: no penalty): bit v & 31 of word v >> 5 of row b says that id v is in row b's own sequence (its
//           unpadded prompt and what it emitted while unfinished).  The logit of such an id becomes bf16(x * pen) when x < 0, else
//           bf16(x / pen) (fp32, correctly rounded divide, round-to-nearest-even back to bf16; -inf stays -inf, a NaN stays a NaN):
//           a bf16 value again, so the 16-bit keys of the sampled pick stay exact.  Every pass of every pick applies it where it turns
//           a loaded logit into a float, so all passes see the same penalised row.
//   min_new while cnt < min_new, `eos` is no candidate.
// After the pick thread 0 of the row's block sets the emitted token's bit, unless the row had finished before this step: one block owns
// one row, so a plain load-or-store does and nothing depends on the order in which blocks arrive.
struct PickProcs {
    unsigned* seen;
    int seen_ld;
    float pen;
    int min_new;
};
__device__ __forceinline__ float proc_penalise(float x, float pen) {
    return x != x ? x : rbf(x < 0.f ? x * pen : __fdiv_rn(x, pen));
}
__device__ __forceinline__ bool proc_hit(const unsigned* seen_row, int v) { return seen_row && ((seen_row[v >> 5] >> (v & 31)) & 1u); }
__device__ __forceinline__ void proc_mark(const PickProcs& pp, int b, int t, int V) {
    if (pp.seen && t >= 0 && t < V) pp.seen[(long)b * pp.seen_ld + (t >> 5)] |= 1u << (t & 31);
}

// grid B, 1024 threads, 8 logits per load: argmax over the valid vocabulary (ids >= V and the special range are excluded; ties ->
// smallest id, like torch.argmax on the CPU), then HF's bookkeeping: finished rows emit `pad`; a row finishes when it emits `eos`.
constexpr int PICK_T = 1024;
template <bool PROC>
__global__ __launch_bounds__(PICK_T) void decode_pick_kernel(const bf16_t* __restrict__ logits, int ldl, int V, int special0, int nspecial,
                                                             int* __restrict__ state, int* __restrict__ out, int max_steps, int B, int eos,
                                                             int pad, PickProcs pp) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bf16_t* row = logits + (long)b * ldl;
    const unsigned* srow = (PROC && pp.seen) ? pp.seen + (long)b * pp.seen_ld : nullptr;
    const bool ban = PROC && state[7 * B + 2] < pp.min_new;          // `eos` is no candidate yet
    float best = -INFINITY;
    int bi = PICK_NONE, be = 0;
    auto take = [&](float x, int v, bool hit) {
        if (!pick_allowed(v, V, special0, nspecial) || (PROC && ban && v == eos)) return;
        if (PROC && hit) x = proc_penalise(x, pp.pen);
        if (pick_beats(x, v, best, bi)) { best = x; bi = v; }
    };
    const bool vec = ((ldl & 7) == 0) && ((((uintptr_t)logits) & 15) == 0);
    if (vec) {
        for (int v0 = tid * 8; v0 < V; v0 += PICK_T * 8) {
            const u32x4 q = *(const u32x4*)(row + v0);                 // ldl >= V rounded up by the caller's padding (vocab_pad % 8 == 0)
            const unsigned w = srow ? srow[v0 >> 5] >> (v0 & 31) : 0u;  // v0 % 8 == 0: the eight ids share one word (v0 < V: inside seen_ld)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                take(__uint_as_float(q[j] << 16), v0 + 2 * j, (w >> (2 * j)) & 1u);
                take(__uint_as_float(q[j] & 0xffff0000u), v0 + 2 * j + 1, (w >> (2 * j + 1)) & 1u);
            }
        }
    } else {
        for (int v = tid; v < V; v += PICK_T) take(bf2f(row[v]), v, PROC && proc_hit(srow, v));
    }
    pick_reduce<PICK_T, false>(best, bi, be);
    if (tid == 0) {
        const bool was = pick_emit(state, out, max_steps, B, b, bi, eos, pad);
        if (PROC && !was) proc_mark(pp, b, bi, V);
    }
}

// The same pick over the CHILDREN of a trie node (TrieLogitsProcessor, models/modified_lm.py:10-30, with the trie flattened by
// kvcache.flatten_trie): grid B, 256 threads striding over the edges [off[n], off[n+1]) of the sample's node n = node[b]; edge e
// carries the token tok[e] and the node nxt[e] it leads to.  The row then moves to the winning edge's node -- unless it had already
// finished, which leaves node[b] alone (it emits `pad`).  A leaf is one edge `eos -> itself`, so it needs no case of its own.
// Nothing is read or written out of bounds whatever the tables hold: a node outside [0, n_nodes), edges outside [0, off[n_nodes]),
// token ids < 0 and successors outside [0, n_nodes) are skipped.  A node that is left with NO pickable child (all >= V or special;
// kvcache.py keeps such tries on the host loop) emits `eos`, which finishes the row, and keeps its node.
constexpr int TRIE_T = 256;
template <bool PROC>
__global__ __launch_bounds__(TRIE_T) void decode_pick_trie_kernel(const bf16_t* __restrict__ logits, int ldl, int V, int special0,
                                                                  int nspecial, const int* __restrict__ toff, const int* __restrict__ ttok,
                                                                  const int* __restrict__ tnxt, int n_nodes, int* __restrict__ node,
                                                                  int* __restrict__ state, int* __restrict__ out, int max_steps, int B,
                                                                  int eos, int pad, PickProcs pp) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bf16_t* row = logits + (long)b * ldl;
    const unsigned* srow = (PROC && pp.seen) ? pp.seen + (long)b * pp.seen_ld : nullptr;     // (min_new is refused with a trie)
    const int n = node[b];
    int e0 = 0, e1 = 0;
    if (n >= 0 && n < n_nodes) {
        const int E = toff[n_nodes];
        e0 = max(toff[n], 0);
        e1 = min(toff[n + 1], E);
    }
    float best = -INFINITY;
    int bi = PICK_NONE, be = -1;
    for (int e = e0 + tid; e < e1; e += TRIE_T) {
        const int v = ttok[e];
        if (v < 0 || !pick_allowed(v, V, special0, nspecial)) continue;
        float x = bf2f(row[v]);
        if (PROC && proc_hit(srow, v)) x = proc_penalise(x, pp.pen);
        if (pick_beats(x, v, best, bi)) { best = x; bi = v; be = e; }
    }
    pick_reduce<TRIE_T, true>(best, bi, be);
    if (tid == 0) {
        const bool none = bi == PICK_NONE;
        const bool was = pick_emit(state, out, max_steps, B, b, none ? eos : bi, eos, pad);
        if (PROC && !was) proc_mark(pp, b, none ? eos : bi, V);
        if (!was && !none) {
            const int m = tnxt[be];
            if (m >= 0 && m < n_nodes) node[b] = m;
        }
    }
}

// ---- sampled decoding (HF sample() as the host loop of kvcache.py restates it: mask -> trie -> / temperature -> top-k -> top-p ->
// softmax -> one draw per row).  Grid B, 1024 threads.  The ITEMS of row b are the ids [0, V) (TRIE = false) or the edges of node[b], which are
// sorted by token id (TRIE = true, with the bounds handling of decode_pick_trie_kernel); an item is a CANDIDATE when its id passes
// pick_allowed and its logit is no NaN.
//   top-k   x_k = the top_k-th largest candidate logit (with multiplicity); every candidate >= x_k is kept (ties at the threshold
//           included, as `lg < kth` does on the host); top_k == 0 or >= the number of candidates keeps them all.  Logits are bf16, so
//           x_k is found exactly by a two-pass radix select over the order-preserving 16-bit key: two 256-bin LDS histograms, no sort.
//   weight  w = exp((x - m) / T) in fp32, m = the largest candidate logit (always kept): the total is >= 1; w(-inf) = 0.
//   top-p   (HF's TopPLogitsWarper after top-k; top_p >= 1: off, the two passes below are skipped)  a logit value x stays iff the
//           weight S(x) of the top-k survivors with a STRICTLY larger logit is < top_p * W, W their total; candidates that share a
//           logit value stay or go together (HF breaks an exact tie at the boundary by sort order), the class of the maximum always
//           stays (S = 0).  The smallest staying key is found like x_k, by two more passes over the row (high byte, then low byte
//           inside the boundary bin) whose histograms hold weight MASS instead of counts: floor(w * 2^40) as a 64-bit integer, added
//           with integer LDS atomics -- integer adds commute, so the masses and with them the boundary do not depend on the order
//           in which threads arrive (no floating-point atomics anywhere).  V <= 2^23 keeps the total below 2^63; the truncation
//           loses < V * 2^-40 of a total >= 1.  S and W are compared as (double)S < (double)top_p * (double)W.
//   draw    u = philox_u01(word 0 of Philox counter rng[1] + cnt*B + b, key rng[0]); the pick is the first kept item whose running sum
//           of weights, in item order, exceeds u * total -- past the end (rounding): the last kept item with w > 0.  Each thread owns
//           a contiguous item range and sums it in order; a block scan of the 1024 sums gives every range its start.  The order is
//           fixed, so equal (logits, rng, cnt) give equal tokens, eager or replayed.
// The four (top-p: six) passes re-read the row (64 KB at V = 32 000: L2-resident right after the lm_head wrote it); the histogram
// passes stride over the items, the two summing passes walk each thread's own range.  A row without a kept candidate of non-zero
// weight emits `eos` and keeps its node.  kept_out (nullable): kept_out[cnt*B + b] = the number of candidates kept by both warpers, 0
// for such an `eos` row; finished rows write none.  Nothing outside logits[b, 0..V), the tables and state/out/u_out/kept_out[cnt*B + b]
// is touched.
constexpr int SAMP_T = 1024;
// inclusive scan over the SAMP_T threads (in each wave, then over the 16 wave totals in wave order); `total` to every thread
template <typename T>
__device__ __forceinline__ T samp_scan(T v, T& total) {
    __shared__ T ws[SAMP_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    __syncthreads();                                                  // (the readers of an earlier scan are done with ws)
    if (lane == 63) ws[w] = v;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < SAMP_T / 64; ++j) {
        if (j < w) base += ws[j];
        total += ws[j];
    }
    return base + v;
}
// the bin of a 256-bin histogram that holds the k-th largest entry (1 <= k <= the histogram's total), and k's rank inside that bin
__device__ __forceinline__ void samp_select(const int* hist, int k, int* bin, int* rank, int& total) {
    const int tid = threadIdx.x;
    const int c = tid < 256 ? hist[255 - tid] : 0;                    // thread t holds bin 255 - t: the scan counts from the top
    const int above = samp_scan<int>(c, total) - c;
    if (tid < 256 && above < k && above + c >= k) { *bin = 255 - tid; *rank = k - above; }
    __syncthreads();
}
// the same for a histogram of weight masses: the bin in which `above0` + the mass counted from the top first reaches top_p * W (W == 0:
// this histogram's total), and the mass above that bin.  Selects nothing when the histogram is empty.
__device__ __forceinline__ void samp_select_mass(const unsigned long long* mass, unsigned long long above0, float top_p, unsigned long long W,
                                                 int* bin, unsigned long long* above, unsigned long long& total) {
    const int tid = threadIdx.x;
    const unsigned long long c = tid < 256 ? mass[255 - tid] : 0ull;
    const unsigned long long upto = above0 + samp_scan<unsigned long long>(c, total);
    const double lim = (double)top_p * (double)(W ? W : total);
    if (tid < 256 && c > 0 && (double)(upto - c) < lim && (double)upto >= lim) { *bin = 255 - tid; *above = upto - c; }
    __syncthreads();
}
constexpr float SAMP_MASS_ONE = 1099511627776.f;                      // 2^40: the fixed-point unit of the top-p masses
template <bool TRIE, bool PROC>
__global__ __launch_bounds__(SAMP_T) void decode_pick_sample_kernel(const bf16_t* __restrict__ logits, int ldl, int V, int special0,
                                                                    int nspecial, const int* __restrict__ toff, const int* __restrict__ ttok,
                                                                    const int* __restrict__ tnxt, int n_nodes, int* __restrict__ node,
                                                                    float temperature, int top_k, float top_p,
                                                                    const uint64_t* __restrict__ rng, float* __restrict__ u_out,
                                                                    int* __restrict__ kept_out, int* __restrict__ state,
                                                                    int* __restrict__ out, int max_steps, int B, int eos, int pad,
                                                                    PickProcs pp) {
    __shared__ int hist[2][256];
    __shared__ unsigned long long mass[2][256], s_above[2];
    __shared__ int s_bin[2], s_rank[2], s_pbin[2], s_max, s_first, s_last, s_kept;
    __shared__ float s_u;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bf16_t* row = logits + (long)b * ldl;
    if (tid == 0) {
        const int cnt = state[7 * B + 2];
        const uint64_t ctr = rng[1] + (uint64_t)(long)cnt * (uint64_t)B + (uint64_t)b;
        uint32_t r[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)rng[0], (uint32_t)(rng[0] >> 32), r);
        s_u = philox_u01(r[0]);
        if (u_out && cnt >= 0 && cnt < max_steps) u_out[(long)cnt * B + b] = s_u;
        s_max = -1; s_first = PICK_NONE; s_last = -1; s_kept = 0;
        s_bin[0] = s_bin[1] = 0; s_rank[0] = s_rank[1] = 0;
        s_pbin[0] = s_pbin[1] = 0; s_above[0] = s_above[1] = 0;
    }
    if (state[B + b] != 0) {                                          // a finished row emits `pad` whatever it would draw (fin[b] is
        if (tid == 0) pick_emit(state, out, max_steps, B, b, pad, eos, pad);   // written by this block's thread 0 alone)
        return;
    }
    const unsigned* srow = (PROC && pp.seen) ? pp.seen + (long)b * pp.seen_ld : nullptr;
    const bool ban = PROC && state[7 * B + 2] < pp.min_new;          // `eos` is no candidate yet (cnt moves in decode_advance_kernel only)
    int e0 = 0, n = V;
    if (TRIE) {
        const int nd = node[b];
        int e1 = 0;
        if (nd >= 0 && nd < n_nodes) {
            const int E = toff[n_nodes];
            e0 = max(toff[nd], 0);
            e1 = min(toff[nd + 1], E);
        }
        n = max(e1 - e0, 0);
    }
    // item i -> its id v and the order-preserving key of its logit (larger logit <=> larger key; -0 counts as +0), -1: no candidate
    auto key_of = [&](int i, int& v) -> int {
        v = TRIE ? ttok[e0 + i] : i;
        if (v < 0 || !pick_allowed(v, V, special0, nspecial) || (PROC && ban && v == eos)) return -1;
        uint32_t h = row[v];
        if (PROC && proc_hit(srow, v)) h = f2bf(proc_penalise(bf2f((bf16_t)h), pp.pen));
        if ((h & 0x7fffu) > 0x7f80u) return -1;                       // NaN
        if (h == 0x8000u) h = 0;
        return (int)((h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u));
    };
    auto logit_of = [](int key) -> float { return bf2f((bf16_t)((key & 0x8000) ? (key & 0x7fff) : (~key & 0xffff))); };
    if (tid < 256) hist[0][tid] = hist[1][tid] = 0;
    __syncthreads();
    // pass 1: the histogram of the keys' high bytes, the number of candidates and the largest key
    int v, kmax = -1;
    for (int i = tid; i < n; i += SAMP_T) {
        const int k = key_of(i, v);
        if (k < 0) continue;
        atomicAdd(&hist[0][k >> 8], 1);
        kmax = max(kmax, k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o, 64));
    if ((tid & 63) == 0) atomicMax(&s_max, kmax);
    __syncthreads();
    int ncand, dummy;
    const int want = top_k > 0 ? top_k : 0x7fffffff;
    samp_select(hist[0], want, &s_bin[0], &s_rank[0], ncand);        // (selects nothing when want > ncand)
    int thr = 0;                                                      // the smallest kept key
    if (want < ncand) {
        // pass 2: the low bytes of the keys that share the threshold's high byte
        const int hb = s_bin[0];
        for (int i = tid; i < n; i += SAMP_T) {
            const int k = key_of(i, v);
            if (k >= 0 && (k >> 8) == hb) atomicAdd(&hist[1][k & 255], 1);
        }
        __syncthreads();
        samp_select(hist[1], s_rank[0], &s_bin[1], &s_rank[1], dummy);
        thr = (hb << 8) | s_bin[1];
    }
    const float m = logit_of(max(s_max, 0)), T = temperature;
    auto weight_of = [&](int k) -> float {
        if (k < thr) return 0.f;
        const float x = logit_of(k);
        return x == -INFINITY ? 0.f : x == m ? 1.f : expf((x - m) / T);
    };
    if (top_p < 1.f) {
        // top-p pass 1: the weight mass of the top-k survivors per high byte
        if (tid < 256) mass[0][tid] = mass[1][tid] = 0;
        __syncthreads();
        auto mass_of = [&](int k) -> unsigned long long { return (unsigned long long)(weight_of(k) * SAMP_MASS_ONE); };
        for (int i = tid; i < n; i += SAMP_T) {
            const int k = key_of(i, v);
            const unsigned long long q = k < 0 ? 0ull : mass_of(k);
            if (q) atomicAdd(&mass[0][k >> 8], q);
        }
        __syncthreads();
        unsigned long long W, sub;
        samp_select_mass(mass[0], 0ull, top_p, 0ull, &s_pbin[0], &s_above[0], W);
        if (W > 0) {                                                  // (W == 0: nothing weighs anything, the row emits `eos`)
            // top-p pass 2: the same per low byte inside the boundary's high byte
            const int hb = s_pbin[0];
            for (int i = tid; i < n; i += SAMP_T) {
                const int k = key_of(i, v);
                const unsigned long long q = (k >= 0 && (k >> 8) == hb) ? mass_of(k) : 0ull;
                if (q) atomicAdd(&mass[1][k & 255], q);
            }
            __syncthreads();
            samp_select_mass(mass[1], s_above[0], top_p, W, &s_pbin[1], &s_above[1], sub);
            thr = max(thr, (hb << 8) | s_pbin[1]);                    // (the boundary bin holds a top-k survivor: it is >= thr already)
        }
    }
    // pass 3: each thread sums the weights of its own contiguous items, in order
    const int per = (n + SAMP_T - 1) / SAMP_T;
    const int i0 = (int)min((long)tid * per, (long)n), i1 = (int)min((long)i0 + per, (long)n);
    float mine = 0.f;
    int kept = 0;
    for (int i = i0; i < i1; ++i) {
        const int k = key_of(i, v);
        mine += weight_of(k);
        kept += k >= thr;                                             // (no candidate: k = -1 < thr)
    }
    if (kept_out) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
        if ((tid & 63) == 0) atomicAdd(&s_kept, kept);
    }
    float total;
    float run = samp_scan<float>(mine, total) - mine;                 // the running sum in front of item i0
    // pass 4: the same sums again, against u * total
    const float target = s_u * total;
    int first = PICK_NONE, last = -1;
    for (int i = i0; i < i1; ++i) {
        const float w = weight_of(key_of(i, v));
        if (w > 0.f) {
            run += w;
            last = i;
            if (first == PICK_NONE && run > target) first = i;
        }
    }
    if (first != PICK_NONE) atomicMin(&s_first, first);
    if (last >= 0) atomicMax(&s_last, last);
    __syncthreads();
    if (tid == 0) {
        const int i = s_first != PICK_NONE ? s_first : s_last;
        const bool none = i < 0;
        if (!none) key_of(i, v);
        pick_emit(state, out, max_steps, B, b, none ? eos : v, eos, pad);
        if (PROC) proc_mark(pp, b, none ? eos : v, V);                // (a finished row has returned above)
        const int cnt = state[7 * B + 2];
        if (kept_out && cnt >= 0 && cnt < max_steps) kept_out[(long)cnt * B + b] = none ? 0 : s_kept;
        if (TRIE && !none) {
            const int nx = tnxt[e0 + i];
            if (nx >= 0 && nx < n_nodes) node[b] = nx;
        }
    }
}

// one block: the token picked for sample b goes to cache row b*cap + len[b] at position len[b]; dyn = {max len + 1, 128-aligned
// first query row}; len += 1; cnt += 1.  A full cache (len == cap) sends the row to the junk row B*cap, stops growing, marks the sample
// FINISHED (it emits `pad` from the next step on: its query would be read back from the shared junk row, i.e. be garbage) and
// raises the sticky `overflow` word (unless the sample had already finished), which the host must check -- a full cache is an error
// of the caller, not a silent wrong answer.
__global__ __launch_bounds__(64) void decode_advance_kernel(int* __restrict__ state, int B, int cap) {
    __shared__ int smax, smin;
    const int tid = threadIdx.x;
    if (tid == 0) { smax = 0; smin = 0x7fffffff; }
    __syncthreads();
    int* len = state + 2 * B;
    int* pos = state + 3 * B;
    int* crow = state + 4 * B;
    int* grow = state + 5 * B;
    int* last = state + 6 * B;
    for (int b = tid; b < B; b += 64) {
        const int L = len[b];
        const bool full = L >= cap;
        const int Lc = full ? cap - 1 : L;
        pos[b] = Lc;
        crow[b] = full ? B * cap : b * cap + L;
        grow[b] = b * cap + Lc;
        last[b] = b;
        if (!full) len[b] = L + 1;
        else {
            // a row that had ALREADY finished (eos) only emits `pad` from here on: its cache filling up while other samples still
            // decode is not an error -- every token it emitted is valid
            if (!state[B + b]) state[7 * B + 3] = 1;
            state[B + b] = 1;
        }
        atomicMax(&smax, Lc);
        atomicMin(&smin, Lc);
    }
    __syncthreads();
    if (tid == 0) {
        state[7 * B] = smax + 1;
        state[7 * B + 1] = (smin / 128) * 128;
        state[7 * B + 2] += 1;
    }
}

}  // namespace

extern "C" {

int nv_decode_state_ints(int B) { return B > 0 ? 7 * B + 4 : 0; }

// The one pick entry (include/navillm_hip_procs.h): greedy or sampled, over the vocabulary or over a trie node's children, with or
// without the processors.  The four entries below are calls of it with the processors off, which launch the PROC = false kernels.
int nv_decode_pick_proc_bf16(const void* logits, int ldl, int V, int special0, int nspecial, const int* trie_off, const int* trie_tok,
                             const int* trie_nxt, int n_nodes, int* node, int sample, float temperature, int top_k, float top_p,
                             const unsigned long long* rng, float* u_out, int* kept_out, unsigned* seen, int seen_ld, float rep_penalty,
                             int min_new, int* state, int* out, int max_steps, int B, int eos, int pad, void* stream) {
    if (!logits || !state || !out || B <= 0 || V <= 0 || ldl < V || max_steps < 0 || nspecial < 0) return NV_ERR_ARG;
    const bool trie = trie_off || trie_tok || trie_nxt || node || n_nodes != 0;
    if (trie && (!trie_off || !trie_tok || !trie_nxt || !node || n_nodes <= 0)) return NV_ERR_ARG;
    if (sample) {
        if (!rng) return NV_ERR_ARG;
        if (!(temperature > 0.f && temperature <= 3.402823466e38f) || top_k < 0) return NV_ERR_ARG;  // (a NaN fails both comparisons)
        if (!(top_p > 0.f && top_p <= 1.f)) return NV_ERR_ARG;                                       // (so does this one)
        if (top_p < 1.f && V > (1 << 23)) return NV_ERR_ARG;                                         // the 64-bit masses: V * 2^40 < 2^63
    }
    if (!(rep_penalty > 0.f && rep_penalty <= 3.402823466e38f) || min_new < 0) return NV_ERR_ARG;
    if (rep_penalty != 1.f && !seen) return NV_ERR_ARG;
    if (seen && seen_ld < (V + 31) / 32) return NV_ERR_ARG;
    if (min_new > 0 && trie) return NV_ERR_ARG;                       // a trie leaf allows `eos` alone: the trie decides where an answer ends
    const bool proc = seen || min_new > 0;
    const PickProcs pp = {seen, seen_ld, rep_penalty, min_new};
    const bf16_t* lg = (const bf16_t*)logits;
    const uint64_t* r = (const uint64_t*)rng;
    hipStream_t st = (hipStream_t)stream;
#define NV_PICK_GREEDY(K, NT, ...) NV_LAUNCH(K, dim3(B), dim3(NT), 0, st, lg, ldl, V, special0, nspecial, __VA_ARGS__)
#define NV_PICK_SAMPLE(K) \
    NV_LAUNCH(K, dim3(B), dim3(SAMP_T), 0, st, lg, ldl, V, special0, nspecial, trie_off, trie_tok, trie_nxt, n_nodes, node, temperature, top_k, \
              top_p, r, u_out, kept_out, state, out, max_steps, B, eos, pad, pp)
    if (sample) {
        if (trie && proc) NV_PICK_SAMPLE((decode_pick_sample_kernel<true, true>));
        else if (trie) NV_PICK_SAMPLE((decode_pick_sample_kernel<true, false>));
        else if (proc) NV_PICK_SAMPLE((decode_pick_sample_kernel<false, true>));
        else NV_PICK_SAMPLE((decode_pick_sample_kernel<false, false>));
    } else if (trie) {
        if (proc) NV_PICK_GREEDY(decode_pick_trie_kernel<true>, TRIE_T, trie_off, trie_tok, trie_nxt, n_nodes, node, state, out, max_steps, B, eos, pad, pp);
        else NV_PICK_GREEDY(decode_pick_trie_kernel<false>, TRIE_T, trie_off, trie_tok, trie_nxt, n_nodes, node, state, out, max_steps, B, eos, pad, pp);
    } else {
        if (proc) NV_PICK_GREEDY(decode_pick_kernel<true>, PICK_T, state, out, max_steps, B, eos, pad, pp);
        else NV_PICK_GREEDY(decode_pick_kernel<false>, PICK_T, state, out, max_steps, B, eos, pad, pp);
    }
#undef NV_PICK_GREEDY
#undef NV_PICK_SAMPLE
    return nv_check_launch();
}

int nv_decode_pick_bf16(const void* logits, int ldl, int V, int special0, int nspecial, int* state, int* out, int max_steps, int B, int eos,
                        int pad, void* stream) {
    return nv_decode_pick_proc_bf16(logits, ldl, V, special0, nspecial, nullptr, nullptr, nullptr, 0, nullptr, 0, 0.f, 0, 1.f, nullptr, nullptr,
                                    nullptr, nullptr, 0, 1.0f, 0, state, out, max_steps, B, eos, pad, stream);
}

int nv_decode_pick_trie_bf16(const void* logits, int ldl, int V, int special0, int nspecial, const int* trie_off, const int* trie_tok,
                             const int* trie_nxt, int n_nodes, int* node, int* state, int* out, int max_steps, int B, int eos, int pad,
                             void* stream) {
    if (!trie_off || !trie_tok || !trie_nxt || !node || n_nodes <= 0) return NV_ERR_ARG;
    return nv_decode_pick_proc_bf16(logits, ldl, V, special0, nspecial, trie_off, trie_tok, trie_nxt, n_nodes, node, 0, 0.f, 0, 1.f, nullptr,
                                    nullptr, nullptr, nullptr, 0, 1.0f, 0, state, out, max_steps, B, eos, pad, stream);
}

int nv_decode_pick_sample_topp_bf16(const void* logits, int ldl, int V, int special0, int nspecial, const int* trie_off, const int* trie_tok,
                                    const int* trie_nxt, int n_nodes, int* node, float temperature, int top_k, float top_p,
                                    const unsigned long long* rng, float* u_out, int* kept_out, int* state, int* out, int max_steps, int B,
                                    int eos, int pad, void* stream) {
    return nv_decode_pick_proc_bf16(logits, ldl, V, special0, nspecial, trie_off, trie_tok, trie_nxt, n_nodes, node, 1, temperature, top_k, top_p,
                                    rng, u_out, kept_out, nullptr, 0, 1.0f, 0, state, out, max_steps, B, eos, pad, stream);
}

int nv_decode_pick_sample_bf16(const void* logits, int ldl, int V, int special0, int nspecial, const int* trie_off, const int* trie_tok,
                               const int* trie_nxt, int n_nodes, int* node, float temperature, int top_k, const unsigned long long* rng,
                               float* u_out, int* state, int* out, int max_steps, int B, int eos, int pad, void* stream) {
    return nv_decode_pick_sample_topp_bf16(logits, ldl, V, special0, nspecial, trie_off, trie_tok, trie_nxt, n_nodes, node, temperature, top_k,
                                           1.0f, rng, u_out, nullptr, state, out, max_steps, B, eos, pad, stream);
}

int nv_decode_advance(int* state, int B, int cap, void* stream) {
    if (!state || B <= 0 || cap <= 0) return NV_ERR_ARG;
    NV_LAUNCH(decode_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, B, cap);
    return nv_check_launch();
}

}  // extern "C"
