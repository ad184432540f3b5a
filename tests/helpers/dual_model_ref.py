"""CPU reference of the dual video + audio model above its blocks (LTX2Transformer.callAsFunction, LTX2Transformer.swift:254-392):
patchify, the six AdaLayerNormSingle embedders, the caption projections, the block stack (dual_block_ref.forward) and the two output
heads, composed in numpy f32 from the oracle's primitives (timestep_embedding, linear, silu, gelu_tanh, layer_norm, mask_to_bias).
`replay=True` applies the library's rounding points (csrc/dual_model.h and csrc/dual_block.h list them); `mistake=` builds one
deliberately WRONG variant, which tests/test_dual_model_host.py uses to show that the GPU tests' inputs make each piece visible.
`embed(..., dtype=np.float64)` is the float64 reference of the timestep path. Weights: a dict of module keys -> f32 arrays (weights
[out, in]); block parameters under "transformer_blocks.{i}." as dual_block_ref names them."""
import numpy as np

import dual_block_ref as blocks
import ltx_oracle as oracle

F32 = np.float32
# name, numEmbeddings, stream (LTX2Transformer.swift:74,86,93-104)
EMBEDDERS = (("adaln_single", 6, "video"), ("audio_adaln_single", 6, "audio"), ("av_ca_video_scale_shift_adaln_single", 4, "video"),
             ("av_ca_a2v_gate_adaln_single", 1, "video"), ("av_ca_audio_scale_shift_adaln_single", 4, "audio"),
             ("av_ca_v2a_gate_adaln_single", 1, "audio"))
MISTAKES = tuple("drop:" + e[0] for e in EMBEDDERS) + ("audio_reads_video_timestep", "gate_row_first", "swap_head_video", "swap_head_audio",
                                                         "skip_caption_video", "skip_caption_audio", "swap_contexts")
rel_l2, cosine, update_bound = blocks.rel_l2, blocks.cosine, blocks.update_bound


def top_shapes(Hv, Ha, caption_channels=3840, in_channels=128, out_channels=128, audio_in_channels=128, audio_out_channels=128):
    """Module keys and shapes of the top-level parameters (LTX2Transformer.swift:28-48); the two LayerNorms carry none."""
    Dv, Da = Hv * 128, Ha * 64
    s = {}

    def lin(name, out, inp):
        s[name + ".weight"], s[name + ".bias"] = (out, inp), (out,)

    lin("patchify_proj", Dv, in_channels)
    lin("audio_patchify_proj", Da, audio_in_channels)
    for name, n, stream in EMBEDDERS:
        D = Dv if stream == "video" else Da
        lin(name + ".emb.linear_1", D, 256)
        lin(name + ".emb.linear_2", D, D)
        lin(name + ".linear", n * D, D)
    for name, D in (("caption_projection", Dv), ("audio_caption_projection", Da)):
        lin(name + ".linear_1", D, caption_channels)
        lin(name + ".linear_2", D, D)
    s["scale_shift_table"], s["audio_scale_shift_table"] = (2, Dv), (2, Da)
    lin("proj_out", out_channels, Dv)
    lin("audio_proj_out", audio_out_channels, Da)
    return s


def param_shapes(L, Hv, Ha, **kw):
    s = dict(blocks.param_shapes(L, Hv, Ha))
    s.update(top_shapes(Hv, Ha, **kw))
    return s


def checkpoint_spelling(key):
    """The checkpoint's spelling of a module key: the inverse of mapTransformerKey(includeAudio: true) (ModelDownloader.swift:756-803)."""
    if key.startswith("transformer_blocks."):
        return blocks.checkpoint_spelling(key)
    if key.startswith("patchify_proj."):
        return "proj_in." + key[len("patchify_proj."):]
    if key.startswith("adaln_single.emb."):
        return "time_embed.emb.timestep_embedder." + key[len("adaln_single.emb."):]
    if key.startswith("adaln_single.linear."):
        return "time_embed." + key[len("adaln_single."):]
    return key.replace(".emb.", ".emb.timestep_embedder.")


def module_spelling(key):
    """mapTransformerKey(includeAudio: true), restated: what ltx_dual_model_load documents that it accepts."""
    k = key
    if k.startswith("proj_in."):
        k = "patchify_proj." + k[len("proj_in."):]
    if k.startswith("time_embed.emb.timestep_embedder."):
        k = "adaln_single.emb." + k[len("time_embed.emb.timestep_embedder."):]
    elif k.startswith("time_embed.linear."):
        k = "adaln_single." + k[len("time_embed."):]
    k = k.replace(".emb.timestep_embedder.", ".emb.")
    return (k.replace(".norm_q.", ".q_norm.").replace(".norm_k.", ".k_norm.").replace(".to_out.0.", ".to_out.")
            .replace("ff.net.0.proj.", "ff.project_in.proj.").replace("ff.net.2.", "ff.project_out."))


def synth_weights(L, Hv, Ha, seed=5, **kw):
    """The distributions of ltx_dual_model_init_synthetic (not its values), rounded to bf16."""
    w = blocks.synth_weights(L, Hv, Ha, seed)
    rng = np.random.default_rng(seed + 1000)
    for k, shp in top_shapes(Hv, Ha, **kw).items():
        w[k] = oracle.bf16_round(((0.01 if k.endswith(".bias") else 0.02) * rng.standard_normal(shp)).astype(F32))
    return w


def boost(w, Hv, Ha, seed=9):
    """A random-init model (every weight N(0, 0.02^2)) modulates by a few percent, gates included, and its text context and streams are
    small against its biases: whole pieces could be dropped without moving a velocity. A trained checkpoint modulates at order 1. This
    brings random weights to that regime with bf16-exact changes only - powers of two, and gate biases drawn as bf16 values:
    patchify weights x 4 (streams of order 1), caption linear_2 weights x 8 (contexts of order 2, as dual_block_ref.make_inputs),
    every embedder's output Linear weight x 16 and the two output tables x 16 (scale / shift rows of order 0.3, and they move with the
    timestep), N(0, 1) added to the biases of the two cross-modal scale-shift embedders' output Linears (without it the a2v / v2a
    queries and keys hardly notice their modulation), and gate rows of order 1: dual_block_ref.GATES factors times 1 + N(0, 0.3^2)
    added to the output Linears' gate biases."""
    rng = np.random.default_rng(seed)
    Dv, Da = Hv * 128, Ha * 64
    w = dict(w)
    for k, f in (("patchify_proj.weight", 4), ("audio_patchify_proj.weight", 4), ("caption_projection.linear_2.weight", 8),
                 ("audio_caption_projection.linear_2.weight", 8), ("scale_shift_table", 16), ("audio_scale_shift_table", 16)):
        w[k] = (w[k] * F32(f)).astype(F32)
    for name, _, _ in EMBEDDERS:
        w[name + ".linear.weight"] = (w[name + ".linear.weight"] * F32(16)).astype(F32)
    g = blocks.GATES

    def gate(key, D, row, factor):
        b = w[key].copy()
        b[row * D:(row + 1) * D] += (factor * (1.0 + 0.3 * rng.standard_normal(D))).astype(F32)
        w[key] = oracle.bf16_round(b)

    for name in ("av_ca_video_scale_shift_adaln_single", "av_ca_audio_scale_shift_adaln_single"):  # cross-modal scale / shift rows of order 1
        b = w[name + ".linear.bias"]
        w[name + ".linear.bias"] = oracle.bf16_round((b + rng.standard_normal(b.shape)).astype(F32))
    gate("adaln_single.linear.bias", Dv, 2, g["video_self"])
    gate("adaln_single.linear.bias", Dv, 5, g["video_ff"])
    gate("audio_adaln_single.linear.bias", Da, 2, g["audio_self"])
    gate("audio_adaln_single.linear.bias", Da, 5, g["audio_ff"])
    gate("av_ca_a2v_gate_adaln_single.linear.bias", Dv, 0, g["a2v"])
    gate("av_ca_v2a_gate_adaln_single.linear.bias", Da, 0, g["v2a"])
    return w


def make_inputs(B, Hv, Ha, F, H, W, T_a, S, caption_channels=3840, in_channels=128, audio_in_channels=128, seed=0):
    """The inputs of the GPU tests: bf16 latents N(0, 1), bf16 contexts of scale 4, sigmas that differ per stream AND per batch element,
    int32 masks with a third of the text keys masked, differently per stream."""
    rng = np.random.default_rng(seed)
    d = {"B": B, "F": F, "H": H, "W": W, "T_a": T_a, "S": S, "Hv": Hv, "Ha": Ha}
    d["video_latent"] = oracle.bf16_round(rng.standard_normal((B, F * H * W, in_channels)).astype(F32))
    d["audio_latent"] = oracle.bf16_round(rng.standard_normal((B, T_a, audio_in_channels)).astype(F32))
    d["video_context"] = oracle.bf16_round((4.0 * rng.standard_normal((B, S, caption_channels))).astype(F32))
    d["audio_context"] = oracle.bf16_round((4.0 * rng.standard_normal((B, S, caption_channels))).astype(F32))
    d["video_timesteps"] = np.asarray([0.875, 0.4375, 0.6875, 0.1875, 0.9375, 0.3125, 0.5625, 0.0625][:B], F32)
    d["audio_timesteps"] = np.asarray([0.25, 0.75, 0.0625, 0.5, 0.375, 0.8125, 0.125, 0.625][:B], F32)
    for name in ("video", "audio"):
        m = (rng.random((B, S)) >= 1.0 / 3.0).astype(np.int32)
        m[:, 0] = 1
        d[name + "_mask"] = m
    assert not np.array_equal(d["video_mask"], d["audio_mask"])
    return d


def _lin(x, w, name, dtype):
    if dtype == np.float64:
        return x.astype(np.float64) @ w[name + ".weight"].astype(np.float64).T + w[name + ".bias"].astype(np.float64)
    return oracle.linear(x, w[name + ".weight"], w[name + ".bias"])


def _silu(x, dtype):
    return x / (1.0 + np.exp(-x)) if dtype == np.float64 else oracle.silu(x)


def embedder(w, name, sigma, mult=1000.0, dtype=F32):
    """AdaLayerNormSingle (LTXTimestepEmbedding.swift:62-124) on sigma [B]: (linear(silu(embedded)), embedded)."""
    e = oracle.timestep_embedding(np.asarray(sigma, F32) * F32(mult), 256)
    h = _lin(e, w, name + ".emb.linear_1", dtype)
    emb = _lin(_silu(h, dtype), w, name + ".emb.linear_2", dtype)
    return _lin(_silu(emb, dtype), w, name + ".linear", dtype), emb


def embed(w, inp, mult=1000.0, dtype=F32, mistake=None):
    """The timestep path (LTX2Transformer.swift:272-312): temb_v [B][6][Dv], temb_a [B][6][Da], cross_v [B][5][Dv], cross_a [B][5][Da]
    (rows 0-3 from the scale-shift embedder, row 4 from the gate embedder), embts_v [B][Dv], embts_a [B][Da]."""
    B = inp["B"]
    out = {}
    for name, n, stream in EMBEDDERS:
        sigma = inp[stream + "_timesteps"]
        if mistake == "audio_reads_video_timestep":
            sigma = inp["video_timesteps"]
        ada, emb = embedder(w, name, sigma, mult, dtype)
        if mistake == "drop:" + name:
            ada, emb = np.zeros_like(ada), np.zeros_like(emb)
        out[name] = (ada.reshape(B, n, -1), emb)
    gate_first = mistake == "gate_row_first"
    cat = lambda ss, g: np.concatenate([g, ss] if gate_first else [ss, g], axis=1)  # noqa: E731
    return {"temb_v": out["adaln_single"][0], "temb_a": out["audio_adaln_single"][0],
            "cross_v": cat(out["av_ca_video_scale_shift_adaln_single"][0], out["av_ca_a2v_gate_adaln_single"][0]),
            "cross_a": cat(out["av_ca_audio_scale_shift_adaln_single"][0], out["av_ca_v2a_gate_adaln_single"][0]),
            "embts_v": out["adaln_single"][1], "embts_a": out["audio_adaln_single"][1]}


def caption_projection(w, name, context, replay=False):
    """PixArtAlphaTextProjection (LTXTimestepEmbedding.swift:131-152). replay: f32 accumulation, GELU-tanh on the f32 value, one
    rounding to bf16 for the hidden activation and one for the output."""
    h = oracle.gelu_tanh(oracle.linear(context, w[name + ".linear_1.weight"], w[name + ".linear_1.bias"]))
    if replay:
        h = oracle.bf16_round(h)
    y = oracle.linear(h, w[name + ".linear_2.weight"], w[name + ".linear_2.bias"])
    return oracle.bf16_round(y) if replay else y


def head(w, x, table, embts, proj, swap=False, replay=False, eps=1e-6):
    ss = w[table][None].astype(F32) + embts[:, None, :].astype(F32)  # [B][2][D]
    shift, scale = ss[:, 0][:, None, :], ss[:, 1][:, None, :]
    if swap:
        shift, scale = scale, shift
    n = oracle.layer_norm(x, eps) * (F32(1) + scale) + shift
    if replay:
        n = oracle.bf16_round(n.astype(F32))
    return oracle.linear(n.astype(F32), w[proj + ".weight"], w[proj + ".bias"])


def _widen(context, D):
    """What a forgotten caption projection would hand the blocks: the raw context, tiled or cut to the stream width."""
    reps = -(-D // context.shape[-1])
    return np.tile(context, (1, 1, reps))[..., :D].astype(F32)


def forward(w, L, inp, tabs=None, replay=False, mistake=None, mult=1000.0, eps=1e-6):
    """(video_velocity [B][F*H*W][out_channels], audio_velocity [B][T_a][audio_out_channels])."""
    assert mistake is None or mistake in MISTAKES, mistake
    Hv, Ha = inp["Hv"], inp["Ha"]
    Dv, Da = Hv * 128, Ha * 64
    if tabs is None:
        tabs = blocks.tables(None, inp["F"], inp["H"], inp["W"], inp["T_a"], Hv, Ha)
    xv = oracle.linear(inp["video_latent"], w["patchify_proj.weight"], w["patchify_proj.bias"])
    xa = oracle.linear(inp["audio_latent"], w["audio_patchify_proj.weight"], w["audio_patchify_proj.bias"])
    if replay:  # rounding point 1 of dual_model.h: the streams start as the projection's bf16 value
        xv, xa = oracle.bf16_round(xv), oracle.bf16_round(xa)
    e = embed(w, inp, mult, F32, mistake)
    cv, ca = inp["video_context"], inp["audio_context"]
    if mistake == "swap_contexts":
        cv, ca = ca, cv
    pv = _widen(cv, Dv) if mistake == "skip_caption_video" else caption_projection(w, "caption_projection", cv, replay)
    pa = _widen(ca, Da) if mistake == "skip_caption_audio" else caption_projection(w, "audio_caption_projection", ca, replay)
    b = dict(inp)
    b.update(x_video=xv, x_audio=xa, context_video=pv, context_audio=pa, bias_video=oracle.mask_to_bias(inp["video_mask"]),
             bias_audio=oracle.mask_to_bias(inp["audio_mask"]), temb_video=e["temb_v"].astype(F32), temb_audio=e["temb_a"].astype(F32),
             cross_video_ss=e["cross_v"].astype(F32), cross_audio_ss=e["cross_a"].astype(F32))
    xv, xa = blocks.forward(w, L, b, tabs, replay=replay, eps=eps)
    vv = head(w, xv, "scale_shift_table", e["embts_v"], "proj_out", mistake == "swap_head_video", replay, eps)
    va = head(w, xa, "audio_scale_shift_table", e["embts_a"], "audio_proj_out", mistake == "swap_head_audio", replay, eps)
    return vv.astype(F32), va.astype(F32)
