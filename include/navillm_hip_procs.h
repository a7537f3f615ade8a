/*
 * navillm_hip_procs.h -- HF's repetition penalty and minimum length in the device-side decode loop: the entry points of
 * libnavillm_hip.so that came after navillm_hip.h (119, a number the suite pins) and navillm_hip_topp.h (2, likewise).  Same
 * conventions, same library; navillm_amd/lib.py binds them from PROC_SIGNATURES and raises when one is missing.
 */
#ifndef NAVILLM_HIP_PROCS_H
#define NAVILLM_HIP_PROCS_H
#include "navillm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The logits processors (DESIGN.md §4 "Logits processors" states the rule; they run after the special-id mask and in front of the
 *      trie, temperature, top-k and top-p).  nv_decode_pick_proc_bf16 is THE pick: nv_decode_pick_bf16, nv_decode_pick_trie_bf16 and
 *      nv_decode_pick_sample_topp_bf16 are this call with the processors off (seen = NULL, rep_penalty = 1, min_new = 0).
 *        trie_off / trie_tok / trie_nxt / n_nodes / node   all NULL / 0: the candidates are the vocabulary; else a trie as in
 *                 nv_decode_pick_trie_bf16
 *        sample   0: the argmax (temperature, top_k, top_p, rng, u_out and kept_out are ignored); else the draw of
 *                 nv_decode_pick_sample_topp_bf16
 *        seen     [B, seen_ld] 32-bit words, nullable: bit v & 31 of word v >> 5 of row b is set when id v is in row b's own sequence.
 *                 The logit x of such an id becomes bf16(x * rep_penalty) when x < 0, else bf16(x / rep_penalty) -- fp32 arithmetic,
 *                 a correctly rounded divide, round-to-nearest-even back to bf16, -inf stays -inf, a NaN stays a NaN -- in every pass
 *                 of the pick.  After the pick the emitted token's bit is set, unless the row had finished before this step (it then
 *                 emits `pad` and marks nothing).  With seen given and rep_penalty = 1 the bitmap is kept up and changes no logit.
 *        min_new  while cnt < min_new, `eos` is no candidate.
 *      NV_ERR_ARG, before any launch: rep_penalty not finite or <= 0; min_new < 0; rep_penalty != 1 with seen = NULL; seen with
 *      seen_ld < ceil(V / 32); min_new > 0 with trie tables; sample with rng = NULL; and everything the three entries above refuse.
 *      nv_decoder_proc_step: the decode step of nv_decoder_greedy_step / _trie_step / _sample_topp_step with that pick. */
int nv_decode_pick_proc_bf16(const void* logits, int ldl, int V, int special0, int nspecial, const int* trie_off, const int* trie_tok,
                             const int* trie_nxt, int n_nodes, int* node, int sample, float temperature, int top_k, float top_p,
                             const unsigned long long* rng, float* u_out, int* kept_out, unsigned* seen, int seen_ld, float rep_penalty,
                             int min_new, int* state, int* out, int max_steps, int B, int eos, int pad, void* stream);
int nv_decoder_proc_step(const nv_decoder* p, void* hs, const void* embed, const void* lm_head, int Vp, int V, int special0, int nspecial,
                         const int* trie_off, const int* trie_tok, const int* trie_nxt, int n_nodes, int* node, int sample, float temperature,
                         int top_k, float top_p, const unsigned long long* rng, unsigned* seen, int seen_ld, float rep_penalty, int min_new,
                         void* logits, void* x, int* state, int* out, int max_steps, const int* kv0, void* attn_buf, float* lse, int B, int cap,
                         int eos, int pad, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
