// attn_module.h - LTXAttention at head dim 64 as a loadable unit (reference LTXAttention.swift:160-218 at 32 heads x 64,
// LTXConfig.swift:134-135): the module the dual video+audio block adds four times to the video block - audio self-attention, audio
// text cross-attention and the two cross-modal attentions a2v / v2a (LTX2TransformerBlock.swift:133-163,207-270).
//
// One module owns to_q [inner][Dq], to_k / to_v [inner][Dc], to_out [Dq][inner] (bf16, biases f32) and q_norm / k_norm [inner] (f32),
// inner = heads x 64. Forward, in the reference's order, every step on the device:
//   q = to_q(x), k = to_k(context ?? x), v = to_v(context ?? x)  ->  q_norm / k_norm across the whole row  ->  split RoPE on q with
//   (q_cos, q_sin) and on k with (k_cos, k_sin), or with q's tables when only those are given (the reference's `kPe ?? pe`)  ->
//   softmax(q k^T / 8 + key_bias) v per head  ->  to_out.
//
// Rounding points (the reference computes in f32 from f32 inputs, or in bf16 where the context is bf16):
//   1. x [B][Tq][Dq] f32 and an f32 context are rounded to bf16 ONCE, as GEMM operands (as the DiT rounds its stream).
//   2. q and k leave their projections in f32, are normed and rotated in f32 and rounded to bf16 once; q carries the folded softmax
//      scale (1/8) log2(e) in that one rounding (kAttnQueryPrescale64).
//   3. A bf16 context (the text cross-attention, whose K / V Linears are bf16 x bf16 in the reference): k is rounded to bf16 after
//      the projection and again after the norm, as oracle.attention(kv_bf16=True) models it.
//   4. v is rounded to bf16 by the projection's transposed store (V^T [inner][ldvt], what the attention kernel reads).
//   5. Inside the attention kernel P is rounded to bf16 for the PV product (f32 accumulation); its output is bf16.
//   6. to_out accumulates in f32 and writes f32 [B][Tq][Dq].
// Scratch is owned by the module, grows to the largest shape seen and is reused: nothing is allocated per call.
//
// attn_module_core is the same sequence for a caller that is a block (dual_block.cpp): its query and context rows arrive as bf16,
// already normed and modulated (rounding point 1 is the caller's), the scratch is the caller's, and to_out ends in the gated-residual
// epilogue straight into the caller's f32 stream. A module made by attn_module_create_ex may have 128-wide heads (the video half of
// the dual block) and, for self-attention, to_q and to_k stored as one [2 inner][Dq] matrix so that one GEMM feeds the norm + RoPE
// pass (the DiT's layout). attn_module_forward takes neither: it is unchanged.
#pragma once
#include <map>
#include <string>

#include "dit.h"
#include "runtime.h"

struct AttnModule {
    int heads = 0, inner = 0, Dq = 0, Dc = 0;
    int head_dim = 64;      // 128: attn_module_create_ex only
    bool fused_qk = false;  // to_q | to_k contiguous, q.w [2 inner][Dq] and q.b [2 inner] (attn_module_create_ex, Dc == Dq)
    float eps = 1e-6f;
    LinearW q, k, v, o;
    float* qn = nullptr;
    float* kn = nullptr;
    ParamTable params;  // one arena (two with split_weights); "to_q.weight", "to_q.bias", .., "q_norm.weight", "k_norm.weight"
    DevBuf ws_xb, ws_cb, ws_qraw, ws_kraw, ws_q, ws_k, ws_vt, ws_ao;
};

AttnModule* attn_module_create(int query_dim, int context_dim, int heads);
// split_weights: the four bf16 weights go to params.warena and only the f32 parameters to params.arena, so that an owner that quantises
// the module (dual_model_quantize) can release the bf16 weights; false: one arena, as attn_module_create places them
AttnModule* attn_module_create_ex(int query_dim, int context_dim, int heads, int head_dim, bool fused_qk, bool split_weights);
void attn_module_destroy(AttnModule* m);
void attn_module_init_synthetic(ltx_ctx* ctx, AttnModule* m, uint64_t seed);
// shapes of a module stored under `prefix` (e.g. "transformer_blocks.0.audio_to_video_attn.") in a safetensors file; the file's own
// names (to_out.0, norm_q, norm_k) and the module's (to_out, q_norm, k_norm) are both accepted
void attn_module_file_shape(const std::string& path, const std::string& prefix, int* query_dim, int* context_dim, int* inner);
void attn_module_load(ltx_ctx* ctx, AttnModule* m, const std::string& path, const std::string& prefix);

struct AttnModuleArgs {
    const float* x = nullptr;        // [B][Tq][Dq] f32
    const void* context = nullptr;   // [B][Tk][Dc] f32, or bf16 with context_bf16; null = self-attention (Tk == Tq)
    int context_bf16 = 0;
    int B = 1, Tq = 0, Tk = 0;
    const float* q_cos = nullptr;    // [q_rows][inner/2] f32 or null (no RoPE at all)
    const float* q_sin = nullptr;
    int q_rows = 0;
    const float* k_cos = nullptr;    // [k_rows][inner/2] f32; null with q_cos given: k is rotated with q's tables
    const float* k_sin = nullptr;
    int k_rows = 0;
    const float* key_bias = nullptr; // [B][Tk] f32 additive, reference units ((1 - mask) * -10000), or null
    float* out = nullptr;            // [B][Tq][Dq] f32
};
void attn_module_forward(ltx_ctx* ctx, AttnModule* m, const AttnModuleArgs& a);

// ---- the core a block calls ----
// V^T of one attention of the caller: [B][inner][Tpad] bf16 whose pad columns must be finite. The slot remembers the layout it holds
// and is zeroed (on the stream) when the layout changes.
struct AttnVtSlot {
    DevBuf buf;
    int inner = 0, Tpad = 0, B = 0;
};
// scratch shared by the attentions of one caller, sized by attn_core_reserve for each of them before the first launch
struct AttnCoreScratch {
    DevBuf qraw, kraw, q, k, ao, attn_split;
};
struct AttnCoreArgs {
    const bf16_t* xq = nullptr;    // [B][Tq][Dq] bf16: the normed (and modulated) query rows
    const bf16_t* ctx = nullptr;   // [B][Tk][Dc] bf16 context rows; null = self-attention over xq (Tk == Tq)
    int kv_bf16 = 0;               // text context: k is rounded to bf16 after its projection and after the norm (rounding point 3)
    int B = 1, Tq = 0, Tk = 0;
    const float* q_cos = nullptr;  // [>= Tq][inner/2]; null = no RoPE
    const float* q_sin = nullptr;
    const float* k_cos = nullptr;  // [>= Tk][inner/2]; null with q tables: k uses q's
    const float* k_sin = nullptr;
    const float* key_bias = nullptr;  // [B][Tk] f32 additive or null
    float* x = nullptr;            // [B][Tq][Dq] f32 stream: x += gate * to_out(attention)
    const float* gate = nullptr;   // [B][gate_bstride] rows, Dq valid columns; null = plain residual
    long gate_bstride = 0;
    const int32_t* gate_rowmap = nullptr;  // optional [B*Tq]: gate row of query row m = gate_rowmap[m] (per-token timestep groups)
    float* split_ws = nullptr;     // optional split-K workspace of the GEMMs (floats)
    long split_ws_elems = 0;
    // K and V^T of a context that does not change between calls (attn_module_build_kv made them): both set = the k GEMM, k's norm pass
    // and the V^T GEMMs are skipped and the attention reads these. ctx / kv_bf16 / the key tables are then not read.
    const bf16_t* cached_k = nullptr;   // [B][Tk][inner] bf16, normed
    const bf16_t* cached_vt = nullptr;  // [B][inner][ceil64(Tk)] bf16, pad columns finite
};
// grows the scratch for one attention of these shapes (no launch; may allocate)
void attn_core_reserve(const AttnModule* m, AttnCoreScratch* ws, AttnVtSlot* vt, int B, int Tq, int Tk);
// launches only: the caller has checked its arguments and reserved the scratch
void attn_module_core(ltx_ctx* ctx, AttnModule* m, const AttnCoreArgs& a, AttnCoreScratch* ws, AttnVtSlot* vt);
// K and V^T of one context into caller memory (k_out [B][Tk][inner], vt_out [B][inner][ceil64(Tk)] whose pad columns the caller has made
// finite): exactly the launches attn_module_core runs for them when nothing is cached - the k GEMM into ws->kraw, k's norm (+ RoPE)
// pass, one V^T GEMM per batch element - with the same operands, a.kv_bf16 and the split-K workspace included, so the outputs carry the
// same bits. Reads a.ctx, a.kv_bf16, a.B, a.Tk, the key tables and a.split_ws; not for a fused q|k module. ws->kraw is reserved.
void attn_module_build_kv(ltx_ctx* ctx, AttnModule* m, const AttnCoreArgs& a, AttnCoreScratch* ws, bf16_t* k_out, bf16_t* vt_out);
