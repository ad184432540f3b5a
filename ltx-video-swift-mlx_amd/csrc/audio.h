// audio.h - the audio decode leg (reference Models/AudioVAE/Vocoder.swift:325-361 decodeAudio): audio latent -> AudioVAE.decode ->
// stereo mel -> LTX2Vocoder -> 24 kHz stereo waveform.
//
// Precision contract (the video VAE's, vae.h): weights are rounded to bf16 at load, every convolution operand is bf16, accumulation
// is f32 (v_mfma_f32_16x16x32_bf16), the residual streams are f32. The reference computes in whatever dtype its files carry; that
// cannot be pinned here.
//
// Every convolution of both models - dilated Conv1d, the ConvTransposed1d phases, the height-causal Conv2d - is ONE computation on a
// zero-haloed, channels-last bf16 buffer,
//     out[p][co] = bias[co] + sum_tap sum_ci W[co][tap][ci] * x[p + off(tap)][ci],
// with a table of row offsets (audio_conv.hip). Nothing on this path goes through rocBLAS, MIOpen or torch.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "runtime.h"

enum { ACONV_MAX_TAPS = 16, ACONV_HALO = 32 };  // rows of zero halo on each side of every 1-D operand (>= 5 * (11-1)/2 = 25)
enum { AACT_NONE = 0, AACT_LEAKY = 1, AACT_TANH = 2 };

// One launch of the shifted-row multi-tap GEMM. Output position p in [0, P) reads operand rows p + off[t]; the caller owns the halo:
// every such row must exist (zeros outside the signal). p splits as (h, w) = (p / wp, p % wp) and is stored only when w < wv (the
// 2-D problems run over the padded pitch; 1-D problems pass wp = 1 << 30). Row of the f32 output = (h * opitch + w) * omul + oadd, of
// the bf16 output = (h * bpitch + w) * omul + oadd (a transposed conv's phase r stores to t * stride + r).
struct AConvArgs {
    const bf16_t* x = nullptr;  // operand, row p = x + p * ldx (may point inside a haloed buffer)
    long ldx = 0;
    const bf16_t* w = nullptr;  // [Cout][ntaps][Cin]
    const float* bias = nullptr;  // [Cout] or null
    int P = 0, Cin = 0, Cout = 0, ntaps = 0;
    int off[ACONV_MAX_TAPS] = {0};
    int wp = 1 << 30, wv = 1 << 30;
    int omul = 1, oadd = 0;
    // f32 output: v = acc + bias (+ resid[row][co]) ; f32_act AACT_TANH applies tanh; transposed: out[co * ldo + row]
    const float* resid = nullptr;
    float* out_f32 = nullptr;
    long ldo = 0;
    int opitch = 0, f32_transposed = 0, f32_act = AACT_NONE;
    // bf16 output: the operand the next conv reads, act(v) (AACT_NONE or AACT_LEAKY with `slope`)
    bf16_t* out_bf16 = nullptr;
    long ldb = 0;
    int bpitch = 0, bf16_act = AACT_NONE;
    float slope = 0.1f;
};
// tile: -1 auto, else the output-channel width of the instance (128, 64 or 32). Throws invalidConfiguration on shapes the kernel
// does not take (Cin % 32, ldx % 8, ntaps, a forced tile that does not exist) before anything is launched.
void launch_audio_conv(const AConvArgs& a, int tile, hipStream_t stream);

// ---- row passes (audio_conv.hip) ----
// f32 [H][W][C] -> bf16 interior of the padded [(H+3)][W+2][C] buffer at (h+2, w+1); mode 0: PixelNorm over C (eps 1e-6) + SiLU
// (AudioVAE.swift:23-26,146-152), mode 1: plain cast (the operand of nin_shortcut).
void launch_audio_pn_pad(const float* x, int H, int W, int C, int mode, bf16_t* out, hipStream_t stream);
// nearest-2x upsample of f32 [H][W][C] written as the operand of the causal conv whose first output row is dropped
// (AudioVAE.swift:178-198): bf16 padded [(2H-1)+3][2W+2][C], upsampled row u at padded row u+1 (ONE zero row on top), column v at v+1.
void launch_audio_upsample_pad(const float* x, int H, int W, int C, bf16_t* out, hipStream_t stream);
// latent f32 [Cl][T][Wl] * std[c*Wl+w] + mean[c*Wl+w] (AudioVAE.swift:415-434) -> bf16 padded [(T+3)][Wl+2][Cpad] (channels >= Cl stay 0)
void launch_audio_denorm_pad(const float* latent, const float* mean, const float* stdv, int Cl, int T, int Wl, int Cpad, bf16_t* out,
                             hipStream_t stream);
// mel f32 [2][T][M] -> bf16 rows [T][2*M], channel c*M + m (Vocoder.swift:220-229); out points at row 0 inside the haloed buffer
void launch_audio_mel_pack(const float* mel, int T, int M, bf16_t* out, hipStream_t stream);
// out[r][0..C) = bf16(leaky((a + b + c) / 3, slope)) over dense f32 [rows][C] (Vocoder.swift:242-250 followed by the next consumer's
// LeakyReLU); out rows are ldb apart
void launch_audio_mean3_act(const float* a, const float* b, const float* c, long rows, int C, float slope, bf16_t* out, long ldb,
                            hipStream_t stream);

// ---- models ----
struct AConvW {
    bf16_t* w = nullptr;  // device [cout][ntaps][cin_pad]
    float* b = nullptr;   // device [cout]
    int cout = 0, cin = 0, cin_pad = 0, k = 0;
};
// host-side tensors keyed by file name (PyTorch layouts), what both the loaders and the synthetic initialisers produce
struct AHostTensor {
    std::vector<long> shape;
    std::vector<float> v;
};
typedef std::map<std::string, AHostTensor> AHostWeights;

struct AudioVaeModel {
    int base = 128, latent_ch = 8, out_ch = 2;
    DeviceArena arena;
    struct Res { AConvW c1, c2, sc; bool has_sc = false; };
    AConvW conv_in, conv_out;
    Res mid[2];
    Res up[3][3];     // up[level][block], file order (level 2 runs first)
    AConvW ups[3];    // upsample conv of levels 2 and 1
    float *mean = nullptr, *stdv = nullptr;  // device [latent_ch * 16]
    std::map<std::string, DevBuf> ws;  // named activation buffers; dropped (and their halos re-zeroed on creation) when T changes
    int ws_T = -1;
};
struct VocoderModel {
    int in_ch = 128, hidden = 1024, out_ch = 2;
    DeviceArena arena;
    AConvW conv_in, conv_out;
    struct Up {
        int k = 0, stride = 0, pad = 0, cin = 0, cin_pad = 0, cout = 0;
        float* b = nullptr;
        std::vector<bf16_t*> w;               // per phase: device [cout][ntaps_r][cin_pad]
        std::vector<std::vector<int>> off;    // per phase: row offsets
    } up[5];
    struct Res { AConvW c1[3], c2[3]; int k = 0; } res[15];
    std::map<std::string, DevBuf> ws;
    int ws_T = -1;
};

// taps of phase r of a transposed conv (kernel k, stride s, padding p): torch tap j contributes to output t*s + r from input row
// t + (r + p - j) / s iff (r + p - j) % s == 0. Returns the js; offs gets the row offsets.
std::vector<int> convt_phase_taps(int k, int s, int p, int r, std::vector<int>* offs);
// weights of one phase in the kernel's order: PyTorch ConvTranspose1d weight w (cin, cout, k) -> [cout][js.size()][cin_pad], tap t of the
// slab = torch tap js[t], input channels >= cin zero. The one [Cout][taps][Cin] reorder: the vocoder loader and the
// ltx_op_conv_transpose1d test hook both build their slabs here.
std::vector<float> convt_phase_slab(const float* w, int cin, int cout, int k, const std::vector<int>& js, int cin_pad);

AudioVaeModel* audio_vae_create();
void audio_vae_destroy(AudioVaeModel* m);
void audio_vae_load(ltx_ctx* ctx, AudioVaeModel* m, const std::string& path);
void audio_vae_init_synthetic(ltx_ctx* ctx, AudioVaeModel* m, int base, uint64_t seed);
// latent device f32 [8][T][16] -> mel device f32 [2][max(4T-3,1)][64]
void audio_vae_decode(ltx_ctx* ctx, AudioVaeModel* m, const float* latent, int T, float* mel);

VocoderModel* vocoder_create();
void vocoder_destroy(VocoderModel* m);
void vocoder_load(ltx_ctx* ctx, VocoderModel* m, const std::string& path);
void vocoder_init_synthetic(ltx_ctx* ctx, VocoderModel* m, int hidden, uint64_t seed);
// mel device f32 [2][T][64] -> waveform device f32 [2][240 T]
void vocoder_forward(ltx_ctx* ctx, VocoderModel* m, const float* mel, int T, float* wave);

// ---- pure host ----
int audio_latent_frames(int video_frames, float fps);  // computeAudioLatentFrames (LTXPipeline.swift:530-534)
inline int audio_mel_frames(int T) { return T * 4 - 3 > 1 ? T * 4 - 3 : 1; }
bool write_wav_pcm16(const char* path, const float* waveform, long n, int sample_rate, float gain);  // AudioExporter.swift:19-92
