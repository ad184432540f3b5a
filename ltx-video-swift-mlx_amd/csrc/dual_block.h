// dual_block.h - LTX2TransformerBlock, the dual video + audio block of the reference (LTX2TransformerBlock.swift:174-297), as a
// loadable stack of L blocks with a forward of its own. It takes what LTX2Transformer.callAsFunction hands its blocks - the two
// residual streams, the two text contexts, the adaLN rows of both streams and the cross-modal scale-shift rows - and returns both
// streams. The embedders that produce those rows (audio_adaln_single, av_ca_*), the patchify / output heads and the caption projections
// are dual_model.h, which owns a DualStack and calls dual_forward; the joint loop is dual_denoise.h; the CLI's --audio path is not built.
//
// Modulation inputs are one row per batch element on the audio stream (temb_a [B][6][Da], cross_audio_ss [B][5][Da]) and one row per
// (batch element, timestep GROUP) on the video stream: temb_v [B*G][6][Dv], cross_video_ss [B*G][5][Dv], with video_row_map[b*Tv + t] =
// b*G + group(b, t), as dit_forward has them. That is the reference's per-token form (image-to-video, LTX2Transformer.swift:285-312:
// the adaLN rows AND both cross-modal embedders read the per-token video timesteps) with every distinct row built once. The map picks
// the video adaLN rows and gates of phases 1 and 7, the a2v query / v2a key modulation of the cross-modal norms and the a2v gate.
// G = 1 without a map is one row per batch element: the same launches, the same bits. B * G <= 8. Map entries are the caller's contract.
//
// The eight phases of one block, in the reference's order (x_v [B][Tv][Dv], x_a [B][Ta][Da], both f32, updated in place):
//   1. video self-attention: adaLN rows 0 (shift) / 1 (scale), gate row 2 of scale_shift_table [6][Dv] + temb_v; heads x 128, 3-D RoPE
//   2. audio self-attention: the same at Da with audio_scale_shift_table + temb_a; heads x 64, audio 1-D RoPE
//   3. video text cross-attention on norm2(x_v): plain RMSNorm, no modulation, no gate, no RoPE, masked bf16 context
//   4. audio text cross-attention on audio_norm2(x_a): the same at head dim 64
//   5. a2v: normVCA = audio_to_video_norm(x_v) and normACA = video_to_audio_norm(x_a) are computed ONCE, after phase 4 and before
//      either update. Video queries normVCA * (1 + ca_v[0]) + ca_v[1] over audio keys normACA * (1 + ca_a[0]) + ca_a[1], gated by
//      ca_v[4], added to x_v; cross-modal video-temporal tables on q, audio tables on k
//   6. v2a: audio queries normACA * (1 + ca_a[2]) + ca_a[3] over video keys normVCA * (1 + ca_v[2]) + ca_v[3] (normVCA from BEFORE the
//      a2v update), gated by ca_a[4], added to x_a; the tables swapped. ca_v = scale_shift_table_a2v_ca_video [5][Dv] + cross_video_ss,
//      ca_a = scale_shift_table_a2v_ca_audio [5][Da] + cross_audio_ss
//   7. video FFN: adaLN rows 3 / 4, gate row 5
//   8. audio FFN: the same at Da
// The six RMSNorm modules (norm1-3, audio_norm1-3) and the two cross-modal norms carry no weight in the checkpoint and the reference
// initialises them to ones: no weight is applied, and a tensor under one of those keys in a file counts as `unmatched`.
//
// Rounding points (the reference computes in f32 from f32 streams, in bf16 where the text context is bf16):
//   1. Every adaLN / plain-norm / cross-modal modulated row is computed in f32 and rounded to bf16 ONCE, as a GEMM operand. The two
//      cross-modal norms are one launch (launch_norm_mod2): each stream is read once, normed once and written twice.
//   2. q and k leave their projections in f32, are normed and rotated in f32 and rounded to bf16 once; q carries the folded softmax
//      scale (1/sqrt(head dim)) log2(e) in that one rounding.
//   3. The text contexts are bf16: k is rounded to bf16 after its projection and again after the norm (oracle.attention(kv_bf16=True)).
//      Text-context K / V^T are computed per forward, per block, unless the caller hands in a DualTextCache (below): the same
//      launches run once per prompt by dual_prepare_text, the same bits.
//   4. v is rounded to bf16 by the projection's transposed store; P is rounded to bf16 for the PV product; attention output is bf16.
//   5. The FFN's hidden activation (GELU-tanh) is rounded to bf16, as the DiT rounds it.
//   6. to_out / FFN-down accumulate in f32 and add gate * (acc + bias) to the f32 stream in the GEMM's epilogue. The streams stay f32.
// Unlike dit_forward there is no sequence parallelism, context cache, STG flag, bf16 q|k store or bf16 split-K partial here.
//
// All four RoPE table sets (video 3-D, audio 1-D, cross-modal video-temporal, cross-modal audio) are made inside from (F, H, W) and
// T_a with rope_tables / audio_positions / video_temporal_positions / rope_tables_positions, cached on the stack and rebuilt when
// the shape changes. Scratch grows to the largest shape seen; nothing is allocated per call once it has. Every argument check
// comes before the first launch: a refused forward writes nothing.
// A null key bias IS an all-zero bias: the text cross-attentions then read a resident row of zeros, so both run the same (masked)
// attention kernels and give the same bits. (The head-dim-64 kernel's masked variant adds the bias in the reference's units, which is
// not the unmasked variant's arithmetic bit for bit; letting null select the unmasked kernels is a follow-up that changes that kernel.)
// Measured on an MI355X (profiles/dual_block_bench.txt): one full-width block 1.42 ms against 2.35 ms composed in
// torch bf16; update rel-L2 against the f32 reference 2.7e-3 (narrow) / 3.1e-3 (full width), equal to the CPU replay's.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "attn_module.h"
#include "dit.h"
#include "runtime.h"

struct DualBlockConfig {
    int num_layers = 48;
    int video_heads = 32, video_dim = 4096;  // video_dim == video_heads * 128
    int audio_heads = 32, audio_dim = 2048;  // audio_dim == audio_heads * 64
    int video_context_dim = 4096;            // width of the video text context (videoCrossAttentionDim)
    int audio_context_dim = 2048;            // width of the audio text context (audioCrossAttentionDim)
    float rope_theta = 10000.0f;
    int max_pos[3] = {20, 2048, 2048};       // video 3-D RoPE
    int audio_max_pos = 20;                  // audio and cross-modal 1-D RoPE (audioMaxPos)
    float fps = 24.0f;
    float norm_eps = 1e-6f;
};

struct DualBlock {
    // video half (DiTBlock's roles), audio half (the same at Da, head dim 64), cross-modal
    AttnModule* attn1 = nullptr;        // video self: fused q|k, heads x 128
    AttnModule* attn2 = nullptr;        // video text cross
    AttnModule* audio_attn1 = nullptr;  // audio self: fused q|k, heads x 64
    AttnModule* audio_attn2 = nullptr;  // audio text cross
    AttnModule* a2v = nullptr;          // audio_to_video_attn: video queries, audio keys
    AttnModule* v2a = nullptr;          // video_to_audio_attn: audio queries, video keys
    LinearW ff1, ff2, aff1, aff2;
};

// K (normed) and V^T of the two text cross-attentions of every block, for contexts that do not change between forwards (one prompt):
// ONE allocation, per block [K attn2 [B][S][Dv]] [V^T attn2 [B][Dv][Spad]] [K audio_attn2 [B][S][Da]] [V^T audio_attn2 [B][Da][Spad]],
// Spad = ceil64(S), L * B * (S + Spad) * (Dv + Da) * 2 bytes (2.4 GB at L 48, B 2, S 1024). The pad columns of V^T are zeroed when
// the layout changes. dual_prepare_text fills it; B == 0: empty.
struct DualTextCache {
    DevBuf buf;
    int B = 0, S = 0, Spad = 0;
    long bytes = 0;   // of the layout held (buf may be larger)
    long builds = 0;  // fills since the stack was created
};

struct DualStack {
    DualBlockConfig cfg;
    int L = 0, Dv = 0, Da = 0;
    // [L][6][Dv], [L][6][Da], [L][5][Dv], [L][5][Da]: one tensor per kind so that one launch builds every block's modulation rows
    float* sst_v = nullptr;
    float* sst_a = nullptr;
    float* sst_ca_v = nullptr;
    float* sst_ca_a = nullptr;
    std::vector<DualBlock> blocks;
    // params.arena: FFN biases and the four scale-shift tables (f32); params.warena: FFN weights (bf16); the attention modules own theirs
    ParamTable params;  // "transformer_blocks.{i}.attn1.to_q.weight", ... (module spelling, i from 0)

    // RoPE tables, cached per (F, H, W) / T_a
    DevBuf rope_v_cos, rope_v_sin, rope_a_cos, rope_a_sin, rope_cv_cos, rope_cv_sin, rope_ca_cos, rope_ca_sin;
    int rope_F = 0, rope_H = 0, rope_W = 0, rope_Ta = 0;
    // scratch
    AttnCoreScratch attn_ws;
    AttnVtSlot vt[6];  // V^T of the six attentions of a block (video self, audio self, video text, audio text, a2v, v2a)
    DevBuf ws_vn, ws_vn2, ws_an, ws_an2, ws_ffh, ws_splitk;
    DevBuf mod_v, mod_a, mod_ca_v, mod_ca_a;  // [B][L][6|5][D] f32
    DevBuf zero_bias;  // [B][S] f32 zeros: what a null key bias reads (allocated zeroed, never written)
    DualTextCache text_cache;
    bool use_norm_mod2 = true;  // false: phases 5 / 6 run the four launch_norm_mod passes (bit-equal; tools/bench_dual_block.py A/B)

    ~DualStack();
};

DualStack* dual_create(const DualBlockConfig& cfg);
void dual_destroy(DualStack* m);
void dual_init_synthetic(ltx_ctx* ctx, DualStack* m, uint64_t seed);
// Keys under transformer_blocks.{first_block + i}. of the file fill block i, i < L; the module's and the checkpoint's spellings are
// both accepted (to_out.0, norm_q / norm_k, ff.net.0.proj / ff.net.2: ModelDownloader.swift:756-803). Fills the load report; a tensor
// the stack needs and the file lacks is weightLoadingFailed.
void dual_load(ltx_ctx* ctx, DualStack* m, const std::string& path, int first_block);

struct DualForwardArgs {
    float* x_video = nullptr;              // [B][F*H*W][Dv] f32, in place
    float* x_audio = nullptr;              // [B][T_a][Da] f32, in place
    const bf16_t* ctx_video = nullptr;     // [B][S][video_context_dim] bf16
    const bf16_t* ctx_audio = nullptr;     // [B][S][audio_context_dim] bf16
    const float* bias_video = nullptr;     // [B][S] f32 additive key bias or null
    const float* bias_audio = nullptr;
    const float* temb_video = nullptr;     // [B*n_groups][6][Dv]
    const float* temb_audio = nullptr;     // [B][6][Da]
    const float* cross_video_ss = nullptr; // [B*n_groups][5][Dv]
    const float* cross_audio_ss = nullptr; // [B][5][Da]
    int B = 1, F = 0, H = 0, W = 0, T_a = 0, S = 0;
    unsigned phase_mask = 0;  // measurement seam (tools/bench_dual_block.py): bit p-1 set = run phase p; 0 = all eight
    // optional: phases 3 and 4 read K / V^T from here and skip their k GEMM, k norm and V^T GEMMs; ctx_video / ctx_audio are then not
    // read (they may be null). Its (B, S) must be the call's, or the forward is refused before the first launch.
    const DualTextCache* text_cache = nullptr;
    // timestep groups of the video stream (head comment): device [B*F*H*W] int32 with entries in [0, B*n_groups), or null with one group
    int n_groups = 1;
    const int32_t* video_row_map = nullptr;
};
void dual_forward(ltx_ctx* ctx, DualStack* m, const DualForwardArgs& a);
// Fills m->text_cache from the two projected contexts (ctx_video [B][S][video_context_dim], ctx_audio [B][S][audio_context_dim], bf16):
// per block the launches phases 3 and 4 would run for K and V^T (attn_module_build_kv). Every check comes before the first launch.
void dual_prepare_text(ltx_ctx* ctx, DualStack* m, const bf16_t* ctx_video, const bf16_t* ctx_audio, int B, int S);
