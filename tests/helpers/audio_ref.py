"""Independent torch restatement of the audio decode leg, from PyTorch primitives only (F.conv1d, F.conv_transpose1d, F.conv2d with
explicit F.pad): the audio VAE decoder (reference Models/AudioVAE/AudioVAE.swift) and the HiFi-GAN vocoder (Vocoder.swift). It takes the
same PyTorch-layout tensors that are written to the safetensors files and shares no code with the library.

The seeded builders fix a weight scale, chosen on the CPU, that keeps a comparison against this reference meaningful (checked by
tests/test_audio_host.py::test_reference_conditions): at the end of every stage the f32 activation std stays within [0.1, 10], the
pre-tanh output has std in [0.1, 1.0] and fewer than 1 % of its samples exceed 3 in magnitude. A vanished or saturated output would let
any implementation pass.
"""
import torch
import torch.nn.functional as F

UP_K = (16, 15, 8, 4, 4)       # Vocoder.swift:148-149
UP_S = (6, 5, 2, 2, 2)
RES_K = (3, 7, 11)             # Vocoder.swift:150-151
RES_D = (1, 3, 5)

# weight scale (std = GAIN / sqrt(fan_in)); see the module docstring
G_CONV = 1.0         # plain convs (conv_in, upsample convs, shortcuts)
G_RES1 = 1.4         # first conv of a residual pair (follows an activation that halves the variance)
G_RES2_VAE = 0.7     # second conv of an audio-VAE block (the branch adds to the stream)
G_RES2_VOC = 0.5     # second conv of a vocoder pair
G_UP = 1.4           # transposed convs (follow LeakyReLU)
G_OUT_VAE = 1.0
G_OUT_VOC = 0.5
BIAS_STD = 0.02


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _normal(g, shape, std):
    return torch.randn(shape, generator=g, dtype=torch.float32) * std


def build_audio_vae_weights(base=128, seed=11, with_encoder_keys=False):
    """decoder.* / latents_mean / latents_std in the file layout: Conv2d weights (out, in, kh, kw) under `...conv.weight`."""
    g = _gen(seed)
    w = {}

    def conv(p, co, ci, k, gain):
        w[p + ".conv.weight"] = _normal(g, (co, ci, k, k), gain / (ci * k * k) ** 0.5)
        w[p + ".conv.bias"] = _normal(g, (co,), BIAS_STD)

    def res(p, ci, co):
        conv(p + ".conv1", co, ci, 3, G_RES1)
        conv(p + ".conv2", co, co, 3, G_RES2_VAE)
        if ci != co:
            conv(p + ".nin_shortcut", co, ci, 1, G_CONV)

    top = base * 4
    conv("decoder.conv_in", top, 8, 3, G_CONV)
    res("decoder.mid.block_1", top, top)
    res("decoder.mid.block_2", top, top)
    ch = top
    for level, mult in ((2, 4), (1, 2), (0, 1)):
        co = base * mult
        for b in range(3):
            res(f"decoder.up.{level}.block.{b}", ch, co)
            ch = co
        if level > 0:
            conv(f"decoder.up.{level}.upsample.conv", ch, ch, 3, G_CONV)
    conv("decoder.conv_out", 2, ch, 3, G_OUT_VAE)
    w["latents_mean"] = _normal(g, (128,), 0.1)
    w["latents_std"] = 1.0 + _normal(g, (128,), 0.1).abs()
    if with_encoder_keys:
        w["encoder.conv_in.conv.weight"] = _normal(g, (base, 2, 3, 3), 0.1)
        w["encoder.conv_in.conv.bias"] = _normal(g, (base,), 0.1)
    return w


def build_vocoder_weights(hidden=1024, seed=12):
    """Conv1d weights (out, in, k); upsamplers.N.weight (in, out, k)."""
    g = _gen(seed)
    w = {}

    def conv(p, co, ci, k, gain):
        w[p + ".weight"] = _normal(g, (co, ci, k), gain / (ci * k) ** 0.5)
        w[p + ".bias"] = _normal(g, (co,), BIAS_STD)

    conv("conv_in", hidden, 128, 7, G_CONV)
    ch = hidden
    for i in range(5):
        co = ch // 2
        w[f"upsamplers.{i}.weight"] = _normal(g, (ch, co, UP_K[i]), G_UP / (ch * UP_K[i] / UP_S[i]) ** 0.5)
        w[f"upsamplers.{i}.bias"] = _normal(g, (co,), BIAS_STD)
        ch = co
        for j in range(3):
            for d in range(3):
                conv(f"resnets.{i * 3 + j}.convs1.{d}", ch, ch, RES_K[j], G_RES1)
                conv(f"resnets.{i * 3 + j}.convs2.{d}", ch, ch, RES_K[j], G_RES2_VOC)
    conv("conv_out", 2, ch, 7, G_OUT_VOC)
    return w


def to(w, device=None, dtype=None):
    return {k: v.to(device=device, dtype=dtype) for k, v in w.items()}


# ---------------------------------------------------------------------------------------------------------------
# audio VAE decoder
# ---------------------------------------------------------------------------------------------------------------
def _pixel_norm(x):
    return x / torch.sqrt((x * x).mean(dim=1, keepdim=True) + 1e-6)  # AudioVAE.swift:23-26


def _causal_conv2d(x, w, p):
    wt, b = w[p + ".conv.weight"], w[p + ".conv.bias"]
    k = wt.shape[-1]
    pad = k - 1
    x = F.pad(x, (pad // 2, pad - pad // 2, pad, 0))  # (left, right, top, bottom): all of the height padding on top (:53-57)
    return F.conv2d(x, wt, b)


def _res_block(x, w, p):
    h = _causal_conv2d(F.silu(_pixel_norm(x)), w, p + ".conv1")
    h = _causal_conv2d(F.silu(_pixel_norm(h)), w, p + ".conv2")
    if p + ".nin_shortcut.conv.weight" in w:
        x = _causal_conv2d(x, w, p + ".nin_shortcut")
    return x + h


def audio_vae_decode(w, latent, stages=None):
    """latent (8, T, 16) -> mel (2, max(4T-3, 1), 64) (AudioVAE.swift:407-456). `stages` (a list) receives the stage outputs."""
    T = latent.shape[1]
    x = latent.permute(1, 0, 2).reshape(T, 128)
    x = x * w["latents_std"] + w["latents_mean"]
    x = x.reshape(T, 8, 16).permute(1, 0, 2)[None]
    h = _causal_conv2d(x, w, "decoder.conv_in")
    h = _res_block(h, w, "decoder.mid.block_1")
    h = _res_block(h, w, "decoder.mid.block_2")
    if stages is not None:
        stages.append(h)
    for level in (2, 1, 0):
        for b in range(3):
            h = _res_block(h, w, f"decoder.up.{level}.block.{b}")
        if level > 0:
            h = h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
            h = _causal_conv2d(h, w, f"decoder.up.{level}.upsample.conv")[:, :, 1:, :]  # AudioVAE.swift:178-198
        if stages is not None:
            stages.append(h)
    h = _causal_conv2d(F.silu(_pixel_norm(h)), w, "decoder.conv_out")
    target = max(4 * T - 3, 1)
    return h[0, :, :target, :64]


# ---------------------------------------------------------------------------------------------------------------
# vocoder
# ---------------------------------------------------------------------------------------------------------------
def vocoder_forward(w, mel, stages=None, pre_tanh=None):
    """mel (2, T, 64) -> waveform (2, 240 T) (Vocoder.swift:217-266)."""
    T = mel.shape[1]
    x = mel.permute(0, 2, 1).reshape(1, 128, T)  # channel c * 64 + mel
    x = F.conv1d(x, w["conv_in.weight"], w["conv_in.bias"], padding=3)
    for i in range(5):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, w[f"upsamplers.{i}.weight"], w[f"upsamplers.{i}.bias"], stride=UP_S[i], padding=(UP_K[i] - UP_S[i]) // 2)
        outs = []
        for j in range(3):
            h = x
            k = RES_K[j]
            for d in range(3):
                p = f"resnets.{i * 3 + j}"
                t = F.conv1d(F.leaky_relu(h, 0.1), w[f"{p}.convs1.{d}.weight"], w[f"{p}.convs1.{d}.bias"], padding=RES_D[d] * (k - 1) // 2,
                             dilation=RES_D[d])
                t = F.conv1d(F.leaky_relu(t, 0.1), w[f"{p}.convs2.{d}.weight"], w[f"{p}.convs2.{d}.bias"], padding=(k - 1) // 2)
                h = h + t
            outs.append(h)
        x = (outs[0] + outs[1] + outs[2]) / 3
        if stages is not None:
            stages.append(x)
    x = F.conv1d(F.leaky_relu(x, 0.01), w["conv_out.weight"], w["conv_out.bias"], padding=3)
    if pre_tanh is not None:
        pre_tanh.append(x)
    return torch.tanh(x)[0]


def audio_decode(wv, wg, latent):
    return vocoder_forward(wg, audio_vae_decode(wv, latent))
