"""CPU reference of the dual video + audio transformer block (LTX2TransformerBlock.callAsFunction, LTX2TransformerBlock.swift:174-297):
an f32 numpy restatement of its eight phases composed from the oracle's primitives (linear, rms_norm, apply_split_rope, sdpa,
gelu_tanh, bf16_round) and attn64_ref.module_forward, a `drop=` switch that omits one named phase, a deliberately WRONG variant that
takes normVCA after the a2v update, a numpy replay of the library's rounding points (csrc/dual_block.h lists them), and the inputs the
GPU tests use. Weights: a dict of module keys -> f32 arrays, "transformer_blocks.{i}.attn1.to_q.weight" ... (weights [out, in])."""
import math

import numpy as np

import attn64_ref
import ltx_oracle as oracle

F32 = np.float32
PHASES = ("video_self", "audio_self", "video_text", "audio_text", "a2v", "v2a", "video_ff", "audio_ff")
VIDEO_PHASES = ("video_self", "video_text", "a2v", "video_ff")
AUDIO_PHASES = ("audio_self", "audio_text", "v2a", "audio_ff")
ATTN = ("attn1", "attn2", "audio_attn1", "audio_attn2", "audio_to_video_attn", "video_to_audio_attn")
LN2 = math.log(2.0)


def param_shapes(L, Hv, Ha, ctx_v=None, ctx_a=None):
    """Module keys and shapes of an L-block stack: video Hv x 128, audio Ha x 64."""
    Dv, Da = Hv * 128, Ha * 64
    ctx_v, ctx_a = ctx_v or Dv, ctx_a or Da
    dims = {"attn1": (Dv, Dv, Dv), "attn2": (Dv, ctx_v, Dv), "audio_attn1": (Da, Da, Da), "audio_attn2": (Da, ctx_a, Da),
            "audio_to_video_attn": (Dv, Da, Da), "video_to_audio_attn": (Da, Dv, Da)}  # query dim, context dim, inner
    s = {}
    for i in range(L):
        p = f"transformer_blocks.{i}."
        for a, (dq, dc, inner) in dims.items():
            s[p + a + ".to_q.weight"], s[p + a + ".to_q.bias"] = (inner, dq), (inner,)
            s[p + a + ".to_k.weight"], s[p + a + ".to_k.bias"] = (inner, dc), (inner,)
            s[p + a + ".to_v.weight"], s[p + a + ".to_v.bias"] = (inner, dc), (inner,)
            s[p + a + ".to_out.weight"], s[p + a + ".to_out.bias"] = (dq, inner), (dq,)
            s[p + a + ".q_norm.weight"] = s[p + a + ".k_norm.weight"] = (inner,)
        for f, d in (("ff", Dv), ("audio_ff", Da)):
            s[p + f + ".project_in.proj.weight"], s[p + f + ".project_in.proj.bias"] = (4 * d, d), (4 * d,)
            s[p + f + ".project_out.weight"], s[p + f + ".project_out.bias"] = (d, 4 * d), (d,)
        s[p + "scale_shift_table"], s[p + "audio_scale_shift_table"] = (6, Dv), (6, Da)
        s[p + "scale_shift_table_a2v_ca_video"], s[p + "scale_shift_table_a2v_ca_audio"] = (5, Dv), (5, Da)
    return s


def checkpoint_spelling(key):
    """The checkpoint's spelling of a module key (the inverse of mapTransformerKey, ModelDownloader.swift:790-800)."""
    return (key.replace(".to_out.", ".to_out.0.").replace(".q_norm.", ".norm_q.").replace(".k_norm.", ".norm_k.")
            .replace("ff.project_in.proj.", "ff.net.0.proj.").replace("ff.project_out.", "ff.net.2."))


def synth_weights(L, Hv, Ha, seed=5):
    """The distributions of ltx_dual_blocks_init_synthetic (not its values): Linear weights N(0, 0.02^2), biases N(0, 0.01^2), q / k norm
    weights 1 + N(0, 0.02^2), tables N(0, 0.02^2), rounded to bf16."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shp in param_shapes(L, Hv, Ha).items():
        if k.endswith("_norm.weight"):
            v = 1.0 + 0.02 * rng.standard_normal(shp)
        elif k.endswith(".bias"):
            v = 0.01 * rng.standard_normal(shp)
        else:
            v = 0.02 * rng.standard_normal(shp)
        w[k] = oracle.bf16_round(v.astype(F32))
    return w


def tables(ltx_or_none, F, H, W, T_a, Hv, Ha, theta=10000.0, max_pos=(20, 2048, 2048), audio_max_pos=20, fps=24.0):
    """The four RoPE table sets of LTX2Transformer.swift:136-236 as (cos, sin) pairs from the oracle and attn64_ref (pure Python)."""
    del ltx_or_none
    Ia = Ha * 64
    apos = attn64_ref.audio_positions(T_a)
    vpos = attn64_ref.video_temporal_positions(F, H, W, fps)
    return {"video": oracle.rope_tables(F, H, W, dim=Hv * 128, num_heads=Hv, theta=theta, max_pos=max_pos),
            "audio": attn64_ref.rope_tables_positions(apos, Ia, theta, audio_max_pos),
            "cross_video": attn64_ref.rope_tables_positions(vpos, Ia, theta, audio_max_pos),
            "cross_audio": attn64_ref.rope_tables_positions(apos, Ia, theta, audio_max_pos)}


def make_inputs(B, Hv, Ha, F, H, W, T_a, S, seed=0):
    """The inputs of the GPU tests. Streams N(0, 1); bf16 contexts of scale 2; a third of the text keys masked, differently per stream;
    modulation rows with scale / shift entries N(0, 0.3^2) and GATE entries of order 1 (1 + N(0, 0.3^2) times a per-phase factor chosen
    so that every phase carries a comparable share of its stream's update - tests/test_dual_block_host.py checks that condition)."""
    rng = np.random.default_rng(seed)
    Dv, Da, Tv = Hv * 128, Ha * 64, F * H * W
    d = {"B": B, "F": F, "H": H, "W": W, "T_a": T_a, "S": S, "Hv": Hv, "Ha": Ha}
    d["x_video"] = rng.standard_normal((B, Tv, Dv)).astype(F32)
    d["x_audio"] = rng.standard_normal((B, T_a, Da)).astype(F32)
    d["context_video"] = oracle.bf16_round((2.0 * rng.standard_normal((B, S, Dv))).astype(F32))
    d["context_audio"] = oracle.bf16_round((2.0 * rng.standard_normal((B, S, Da))).astype(F32))
    for name in ("video", "audio"):
        m = (rng.random((B, S)) >= 1.0 / 3.0).astype(F32)
        m[:, 0] = 1
        d["bias_" + name] = ((1 - m) * F32(-10000.0)).astype(F32)
    assert not np.array_equal(d["bias_video"], d["bias_audio"])

    def rows(n, D, gates):
        t = (0.3 * rng.standard_normal((B, n, D))).astype(F32)
        for r, g in gates.items():
            t[:, r] = (g * (1.0 + 0.3 * rng.standard_normal((B, D)))).astype(F32)
        return t

    d["temb_video"] = rows(6, Dv, {2: GATES["video_self"], 5: GATES["video_ff"]})
    d["temb_audio"] = rows(6, Da, {2: GATES["audio_self"], 5: GATES["audio_ff"]})
    d["cross_video_ss"] = rows(5, Dv, {4: GATES["a2v"]})
    d["cross_audio_ss"] = rows(5, Da, {4: GATES["v2a"]})
    return d


# per-phase gate factors of make_inputs (the text cross-attentions have no gate)
GATES = {"video_self": 2.0, "audio_self": 2.0, "a2v": 2.0, "v2a": 2.0, "video_ff": 0.5, "audio_ff": 0.5}


def _sdpa_replay(q, k, v, heads, bias):
    """The attention kernel's rounding points: q carries scale * log2(e), so the scores are base-2 exponents; P = 2^(s - max) is rounded
    to bf16 for the PV product while the denominators sum the f32 P; the output is rounded to bf16."""
    b, tq, hd = q.shape
    tk, d = k.shape[1], hd // heads
    out = np.empty((b, tq, hd), F32)
    for bi in range(b):
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = (q[bi, :, sl].astype(F32) @ k[bi, :, sl].astype(F32).T) * F32(LN2)
            if bias is not None:
                s = s + bias[bi][None, :].astype(F32)
            p = np.exp(s - s.max(-1, keepdims=True)).astype(F32)
            out[bi, :, sl] = (oracle.bf16_round(p) @ v[bi, :, sl].astype(F32)) / p.sum(-1, keepdims=True)
    return oracle.bf16_round(out)


def attention(w, p, x, heads, head_dim, context=None, q_tables=None, k_tables=None, bias=None, kv_bf16=False, replay=False, eps=1e-6):
    """LTXAttention.callAsFunction (LTXAttention.swift:160-218) on already normed / modulated rows. replay: the library's rounding points
    (x and the context as bf16 operands; q, k rounded once after norm + RoPE, q with its folded prescale; v bf16; bf16 P and output)."""
    mw = {n: w[p + n] for n in attn64_ref.PARAMS}
    if not replay:
        if head_dim == 64:
            return attn64_ref.module_forward(mw, x, heads, context=context, q_tables=q_tables, k_tables=k_tables, bias=bias, kv_bf16=kv_bf16, eps=eps)
        ctx = x if context is None else context
        q = oracle.rms_norm(oracle.linear(x, mw["to_q.weight"], mw["to_q.bias"]), mw["q_norm.weight"], eps)
        k = oracle.linear(ctx, mw["to_k.weight"], mw["to_k.bias"])
        v = oracle.linear(ctx, mw["to_v.weight"], mw["to_v.bias"])
        if kv_bf16:
            k, v = oracle.bf16_round(k), oracle.bf16_round(v)
        k = oracle.rms_norm(k, mw["k_norm.weight"], eps)
        if kv_bf16:
            k = oracle.bf16_round(k)
        if q_tables is not None:
            kt = k_tables if k_tables is not None else q_tables
            q = oracle.apply_split_rope(q, q_tables[0][:q.shape[1]], q_tables[1][:q.shape[1]], heads)
            k = oracle.apply_split_rope(k, kt[0][:k.shape[1]], kt[1][:k.shape[1]], heads)
        o = oracle.sdpa(q, k, v, heads, 1.0 / math.sqrt(head_dim), bias)
        return oracle.linear(o, mw["to_out.weight"], mw["to_out.bias"])
    xb = oracle.bf16_round(x)
    cb = xb if context is None else oracle.bf16_round(context)
    q = oracle.rms_norm(oracle.linear(xb, mw["to_q.weight"], mw["to_q.bias"]), mw["q_norm.weight"], eps)
    k = oracle.linear(cb, mw["to_k.weight"], mw["to_k.bias"])
    if kv_bf16:
        k = oracle.bf16_round(k)
    k = oracle.rms_norm(k, mw["k_norm.weight"], eps)
    v = oracle.bf16_round(oracle.linear(cb, mw["to_v.weight"], mw["to_v.bias"]))
    if q_tables is not None:
        kt = k_tables if k_tables is not None else q_tables
        q = oracle.apply_split_rope(q, q_tables[0][:q.shape[1]], q_tables[1][:q.shape[1]], heads)
        k = oracle.apply_split_rope(k, kt[0][:k.shape[1]], kt[1][:k.shape[1]], heads)
    prescale = F32(F32(1.0 / math.sqrt(head_dim)) * F32(1.4426950408889634))
    q = oracle.bf16_round((q * prescale).astype(F32))
    k = oracle.bf16_round(k)
    o = _sdpa_replay(q, k, v, heads, bias)
    return oracle.linear(o, mw["to_out.weight"], mw["to_out.bias"])


def feed_forward(w, p, x, replay=False):
    if not replay:
        return oracle.feed_forward(w, p, x)
    h = oracle.bf16_round(oracle.gelu_tanh(oracle.linear(oracle.bf16_round(x), w[p + "project_in.proj.weight"], w[p + "project_in.proj.bias"])))
    return oracle.linear(h, w[p + "project_out.weight"], w[p + "project_out.bias"])


def block(w, i, xv, xa, inp, tabs, drop=None, replay=False, norm_vca_after_a2v=False, eps=1e-6):
    """One LTX2TransformerBlock. inp: the dict of make_inputs (contexts, biases, modulation rows); tabs: tables(). drop: one of PHASES."""
    assert drop is None or drop in PHASES, drop
    p = f"transformer_blocks.{i}."
    Hv, Ha = inp["Hv"], inp["Ha"]
    one = F32(1)
    norm = lambda x: oracle.rms_norm(x, None, eps)  # noqa: E731
    mv = w[p + "scale_shift_table"][None].astype(F32) + inp["temb_video"]            # [B][6][Dv]
    ma = w[p + "audio_scale_shift_table"][None].astype(F32) + inp["temb_audio"]
    cv = w[p + "scale_shift_table_a2v_ca_video"][None].astype(F32) + inp["cross_video_ss"]  # [B][5][Dv]
    ca = w[p + "scale_shift_table_a2v_ca_audio"][None].astype(F32) + inp["cross_audio_ss"]
    row = lambda t, r: t[:, r][:, None, :]  # noqa: E731
    if drop != "video_self":
        n = norm(xv) * (one + row(mv, 1)) + row(mv, 0)
        xv = xv + attention(w, p + "attn1.", n, Hv, 128, q_tables=tabs["video"], replay=replay, eps=eps) * row(mv, 2)
    if drop != "audio_self":
        n = norm(xa) * (one + row(ma, 1)) + row(ma, 0)
        xa = xa + attention(w, p + "audio_attn1.", n, Ha, 64, q_tables=tabs["audio"], replay=replay, eps=eps) * row(ma, 2)
    if drop != "video_text":
        xv = xv + attention(w, p + "attn2.", norm(xv), Hv, 128, context=inp["context_video"], bias=inp["bias_video"], kv_bf16=True, replay=replay, eps=eps)
    if drop != "audio_text":
        xa = xa + attention(w, p + "audio_attn2.", norm(xa), Ha, 64, context=inp["context_audio"], bias=inp["bias_audio"], kv_bf16=True, replay=replay,
                            eps=eps)
    nv, na = norm(xv), norm(xa)  # normVCA / normACA: once, before either update
    if drop != "a2v":
        q = nv * (one + row(cv, 0)) + row(cv, 1)
        c = na * (one + row(ca, 0)) + row(ca, 1)
        xv = xv + attention(w, p + "audio_to_video_attn.", q, Ha, 64, context=c, q_tables=tabs["cross_video"], k_tables=tabs["cross_audio"],
                            replay=replay, eps=eps) * row(cv, 4)
    if norm_vca_after_a2v:  # the mistake the tests must be able to see
        nv = norm(xv)
    if drop != "v2a":
        q = na * (one + row(ca, 2)) + row(ca, 3)
        c = nv * (one + row(cv, 2)) + row(cv, 3)
        xa = xa + attention(w, p + "video_to_audio_attn.", q, Ha, 64, context=c, q_tables=tabs["cross_audio"], k_tables=tabs["cross_video"],
                            replay=replay, eps=eps) * row(ca, 4)
    if drop != "video_ff":
        n = norm(xv) * (one + row(mv, 4)) + row(mv, 3)
        xv = xv + feed_forward(w, p + "ff.", n, replay) * row(mv, 5)
    if drop != "audio_ff":
        n = norm(xa) * (one + row(ma, 4)) + row(ma, 3)
        xa = xa + feed_forward(w, p + "audio_ff.", n, replay) * row(ma, 5)
    return xv.astype(F32), xa.astype(F32)


def forward(w, L, inp, tabs, **kw):
    """L blocks on the streams of `inp`; returns (x_video, x_audio)."""
    xv, xa = inp["x_video"], inp["x_audio"]
    for i in range(L):
        xv, xa = block(w, i, xv, xa, inp, tabs, **kw)
    return xv, xa


def rel_l2(got, want):
    g, r = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(g - r) / np.linalg.norm(r))


def cosine(got, want):
    g, r = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(g @ r / (np.linalg.norm(g) * np.linalg.norm(r)))


def update_bound(replay_rel):
    """Bound of the update out - in on the GPU: twice the rel-L2 of the CPU rounding-point replay against the f32 reference at that shape
    (the factor 2 covers MFMA summation order and the exp2 path, which the replay does not model), never above 3e-2."""
    return min(2.0 * replay_rel, 3e-2)
