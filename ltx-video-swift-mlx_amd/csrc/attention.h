// attention.h - launch interface of the flash attention forward kernel (attention.hip).
#pragma once
#include "common.h"

struct AttnArgs {
    const bf16_t* Q = nullptr;   // [B][Tq][ldq], head h occupies columns h*128 .. h*128+127 (h*64 .. h*64+63 at head_dim 64)
    long ldq = 0, q_bstride = 0;
    const bf16_t* K = nullptr;   // [B][Tk][ldk]
    long ldk = 0, k_bstride = 0;
    const bf16_t* Vt = nullptr;  // [B][H*128][ldvt], keys contiguous, ldvt >= roundup(Tk,64), pad columns finite
    long ldvt = 0, vt_bstride = 0;
    bf16_t* O = nullptr;         // [B][Tq][ldo]
    long ldo = 0, o_bstride = 0;
    const float* bias = nullptr;  // optional additive key mask [B][Tk] (reference: (1-m)*-10000, LTXTransformer.swift:141-156)
    long bias_bstride = 0;
    int B = 0, H = 0, Tq = 0, Tk = 0;
    // 128: the kernels above all, unchanged. 64 (the LTX-2 audio / cross-modal attention, 32 heads x 64): attn64_fwd_kernel; the same
    // layouts with 64 in place of 128 (Vt is [B][H*64][ldvt]), any Tq / Tk, bias and q_prescaled as at 128, never key-split (the
    // workspace fields are ignored). The caller sets `scale` (1/8 at head dim 64).
    int head_dim = 128;
    float scale = 0.08838834764831845f;  // 1/sqrt(128)
    // 1: Q already carries scale * log2(e) (written so by qknorm_rope's out_scale, one rounding to bf16): the scores ARE the base-2
    // exponents and `scale` is ignored. The assembly kernel then runs a stream without its 48 v_mul per key tile; the other
    // kernels run with scale = ln 2. The bias stays in the reference's units (added to score * scale).
    int q_prescaled = 0;
    // head_dim 256 (the Gemma-3 text encoder, attn256_causal_kernel): causal grouped-query attention over left-padded keys. Q / O are
    // [B][T][H*256], K is [B][T][Hkv*256], Vt is [B][Hkv*256][ldvt]; query head h reads K/V head h / (H / Hkv), H % Hkv == 0, Tq == Tk.
    // Query i of batch element b attends keys key_start[b] <= j <= i; output rows i < key_start[b] are zeros. `scale` is the caller's
    // (Gemma: query_pre_attn_scalar^-0.5, not a function of the head dim). No bias, no prescale, no key split.
    int Hkv = 0;                         // 0: H (every kernel but the head-dim-256 one requires that)
    int causal = 0;                      // required at head dim 256, refused elsewhere
    const int32_t* key_start = nullptr;  // device [B] or null (no padding); values are clamped to 0 .. T
    int plain_order = 0;  // 1: workgroups in (query block, head, batch) order instead of the XCD-aware order (A/B measurements only)
    // Key split (few queries against many keys: the cross-attention of a 128-token launch is 32 workgroups walking 16 key tiles each).
    // With a workspace the launcher may divide the keys over up to 8 workgroups per (query block, head): each writes its normalised
    // O to a slice of the workspace plus log2 of its softmax denominators, attn_combine_kernel weights the slices together.
    // attn_split_ws_bytes() says how much a launch can use; null = never split.
    void* split_ws = nullptr;
    long split_ws_bytes = 0;
    // set by the launcher for the kernels (callers leave them alone)
    int key_splits = 1, split_keys = 0;   // number of key ranges, keys per range (a multiple of 64)
    bf16_t* o_part = nullptr;             // [splits][B][Tq][H*128]
    float* lse = nullptr;                 // [splits][B][H][roundup(Tq, 192)]
};
// workspace a key-split launch of this shape would use (0: the launcher would not split it)
long attn_split_ws_bytes(int B, int H, int Tq, int Tk);
int attn_key_splits(int B, int H, int Tq, int Tk);  // the number of key ranges (1 = no split)
// what a producer multiplies q by for q_prescaled: (1 / sqrt(128)) * log2(e)
constexpr float kAttnQueryPrescale = 0.08838834764831845f * 1.4426950408889634f;
// the same for head dim 64: (1 / sqrt(64)) * log2(e)
constexpr float kAttnQueryPrescale64 = 0.125f * 1.4426950408889634f;

// head dim 64: queries per workgroup the launcher picks for a launch of this shape (256, 128 or 64)
int attn64_queries_per_workgroup(int B, int H, int Tq);

void launch_attention(const AttnArgs& args, hipStream_t stream);

// Head-dim-256 attention decode (token generation on a KV cache): one query per head against the first n_keys rows of a cache.
// Query head h reads K/V head h / (Hq / Hkv); at most 4 query heads per K/V head. P stays f32. The keys are cut into splits of 64, one
// workgroup per (split, K/V head); a second small launch combines the splits' (m, l, o) exactly. Cache rows of K and columns of V^T
// at or past n_keys never influence the result, whatever bits they hold: the rows are not read, the columns are replaced by select.
struct AttnDecodeArgs {
    const bf16_t* q = nullptr;   // [Hq * 256]
    const bf16_t* K = nullptr;   // [cap][ldk], K/V head h at columns h * 256 ..
    long ldk = 0;
    const bf16_t* Vt = nullptr;  // [Hkv * 256][ldvt], keys contiguous, ldvt >= roundup(n_keys, 64)
    long ldvt = 0;
    bf16_t* O = nullptr;         // [Hq * 256]
    int Hq = 0, Hkv = 0, n_keys = 0;
    float scale = 0.0625f;
    void* ws = nullptr;          // attn_decode_ws_bytes(Hq, n_keys) bytes, 16-byte aligned
    long ws_bytes = 0;
    // set by the launcher
    float* part_o = nullptr;     // [splits][Hq][256] unnormalised outputs
    float* part_ml = nullptr;    // [splits][Hq][2] maximum, denominator
};
long attn_decode_ws_bytes(int Hq, int n_keys);
void launch_attention_decode(const AttnDecodeArgs& args, hipStream_t stream);
