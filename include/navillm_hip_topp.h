/*
 * navillm_hip_topp.h -- nucleus (top-p) sampling in the device-side decode loop: the entry points of libnavillm_hip.so that came
 * after the 119 of navillm_hip.h (whose number the suite pins: tests/test_sample_decode_cpu.py, tests/test_host_cpu.py).  Same
 * conventions, same library; navillm_amd/lib.py binds them from TOPP_SIGNATURES and raises when one is missing.
 */
#ifndef NAVILLM_HIP_TOPP_H
#define NAVILLM_HIP_TOPP_H
#include "navillm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Top-p (HF's TopPLogitsWarper, after temperature and top-k).  nv_decode_pick_sample_topp_bf16: with W the total weight of the
 *      top-k survivors, a logit value x stays iff the weight of the survivors with a STRICTLY larger logit is < top_p * W; candidates
 *      that share a logit value stay or go together (an exact tie at the boundary is kept whole, where HF breaks it by sort order);
 *      the class of the maximum always stays; the draw then runs over what stayed.  The boundary is found exactly (bf16 logits: a
 *      16-bit key, two more radix passes over integer weight masses, no floating-point atomics), so the token stays a pure function of
 *      (logits, rng, cnt, temperature, top_k, top_p).  top_p = 1 switches the warper off: nv_decode_pick_sample_bf16 is this call with
 *      top_p = 1, kept_out = NULL.  kept_out (nullable): kept_out[cnt*B + b] = the number of candidates both warpers kept while
 *      cnt < max_steps, 0 for a row that emits `eos` for want of a candidate with weight; finished rows write none.  NV_ERR_ARG, before
 *      any launch: the above, top_p NaN or outside (0, 1], top_p < 1 with V > 2^23.  nv_decoder_sample_topp_step:
 *      nv_decoder_sample_step with that pick. */
int nv_decode_pick_sample_topp_bf16(const void* logits, int ldl, int V, int special0, int nspecial, const int* trie_off, const int* trie_tok,
                                    const int* trie_nxt, int n_nodes, int* node, float temperature, int top_k, float top_p,
                                    const unsigned long long* rng, float* u_out, int* kept_out, int* state, int* out, int max_steps, int B,
                                    int eos, int pad, void* stream);
int nv_decoder_sample_topp_step(const nv_decoder* p, void* hs, const void* embed, const void* lm_head, int Vp, int V, int special0, int nspecial,
                                const int* trie_off, const int* trie_tok, const int* trie_nxt, int n_nodes, int* node, float temperature,
                                int top_k, float top_p, const unsigned long long* rng, void* logits, void* x, int* state, int* out,
                                int max_steps, const int* kv0, void* attn_buf, float* lse, int B, int cap, int eos, int pad, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
