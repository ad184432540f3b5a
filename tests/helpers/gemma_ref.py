"""CPU replay of the Gemma-3 text encoder's hidden-state extraction (csrc/gemma.cpp), in numpy: f32 arithmetic with a rounding to
bf16 wherever MLX stores a bf16 array. Written from the text of Gemma3Model.swift (Gemma3Attention, Gemma3MLP, Gemma3DecoderLayer,
Gemma3InnerModel.callAsFunction) and Gemma.RMSNorm / Gemma.clipResidual; the rounding points are listed in DESIGN.md 6i.

Stated difference from the reference: rows of padded positions (i < key_start) leave the attention as zeros here; the reference
holds a uniform average of V there. The connector zeroes those positions, so nothing reads either value."""
import math
from dataclasses import dataclass

import numpy as np

F32 = np.float32


def bf16(x):
    """Round f32 to the nearest bf16 (ties to even), returned as f32."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def bf16_bits(x):
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


@dataclass
class Config:  # Gemma3Config.swift:42-60
    hidden: int = 3840
    layers: int = 48
    intermediate: int = 15360
    heads: int = 16
    head_dim: int = 256
    kv_heads: int = 8
    vocab: int = 262208
    rms_eps: float = 1e-6
    rope_theta: float = 1000000.0
    rope_local_base: float = 10000.0
    query_pre_attn_scalar: float = 256.0
    sliding_window: int = 1024
    sliding_window_pattern: int = 6


def is_global(cfg, layer):
    """Gemma3Model.swift:53: isSliding = (layerIdx + 1) % pattern != 0."""
    return (layer + 1) % cfg.sliding_window_pattern == 0


def gain(w):
    """Gemma.RMSNorm applies 1.0 + weight, formed in the weight's dtype: one rounding to bf16."""
    return bf16(F32(1.0) + np.asarray(w, F32))


def rms_norm(x, w, eps):
    """The mean square as the kernels define it: the f32 squares of bf16 values are exact, their sum is exact in f64 and rounded to
    f32 once; division, square root and reciprocal are f32 operations."""
    x = np.asarray(x, F32)
    ms = (x * x).sum(-1, dtype=np.float64, keepdims=True).astype(F32) / F32(x.shape[-1])
    rstd = F32(1.0) / np.sqrt(ms + F32(eps), dtype=F32)
    return bf16(x * rstd * gain(w))


def norm_residual(r, w, eps, x=None, w2=None):
    """h = bf16(x + bf16(rmsnorm(r) * g)) (h = the norm alone without x); n = bf16(rmsnorm(h) * g2) when w2 is given."""
    h = rms_norm(r, w, eps)
    if x is not None:
        h = bf16(np.asarray(x, F32) + h)
    return h, (rms_norm(h, w2, eps) if w2 is not None else None)


def rope_tables(T, base):
    """cos / sin [T][128] f32: angle = p * base^(-i / 128) at position p, evaluated in f64 and rounded to f32 once (no rope_scaling)."""
    freq = np.exp2(-(np.arange(128, dtype=np.float64) / 128.0) * math.log2(float(F32(base))))
    ang = np.arange(T, dtype=np.float64)[:, None] * freq[None, :]
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def qknorm_rope(x, w, cos, sin, T, eps):
    """x [rows][heads*256]: per head RMS norm with bf16(1 + w), rounded to bf16, then element i pairs with i + 128 (non-traditional
    RoPE) at position row % T; one rounding to bf16."""
    rows = x.shape[0]
    y = rms_norm(np.asarray(x, F32).reshape(rows, -1, 256), w, eps)
    p = np.arange(rows) % T
    c, s = cos[p][:, None, :], sin[p][:, None, :]
    y1, y2 = y[..., :128], y[..., 128:]
    out = np.concatenate([y1 * c - y2 * s, y1 * s + y2 * c], axis=-1)
    return bf16(out).reshape(rows, -1)


def gelu_tanh(x):
    """0.5 x (1 + tanh u), u = sqrt(2/pi) (x + 0.044715 x^3), evaluated in f64 through the identity 0.5 (1 + tanh u) = 1 / (1 + exp(-2u))
    and rounded to f32 once: the literal form loses the digits of 1 + tanh(u) to cancellation for negative x (in f32 all of them below
    x = -6, in f64 below x = -7)."""
    x = np.asarray(x, np.float64)
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)
    return (x / (1.0 + np.exp(-2.0 * u))).astype(F32)


def geglu(gu):
    inter = gu.shape[-1] // 2
    return bf16(bf16(gelu_tanh(gu[..., :inter])) * np.asarray(gu[..., inter:], F32))


def embed(ids, table, hidden):
    """table[ids] * bf16(sqrt(hidden)): the scalar is cast to the embedding's dtype first (62.0 at 3840)."""
    return bf16(np.asarray(table, F32)[ids] * bf16(F32(math.sqrt(hidden))))


def attention(q, k, v, Hq, Hkv, scale, key_start=None):
    """f32 softmax on the given values: q [B][T][Hq*256], k / v [B][T][Hkv*256]; query i attends key_start[b] <= j <= i. Rows below
    key_start are zeros. Not rounded."""
    B, T, _ = q.shape
    out = np.zeros((B, T, Hq * 256), F32)
    g = Hq // Hkv
    for b in range(B):
        ks = 0 if key_start is None else int(key_start[b])
        j = np.arange(T)
        allowed = (j[None, :] <= j[:, None]) & (j[None, :] >= ks)
        for h in range(Hq):
            qh = q[b, :, h * 256:(h + 1) * 256].astype(F32)
            kh = k[b, :, (h // g) * 256:(h // g + 1) * 256].astype(F32)
            vh = v[b, :, (h // g) * 256:(h // g + 1) * 256].astype(F32)
            s = (qh @ kh.T) * F32(scale)
            s = np.where(allowed, s, -np.inf)
            s[:ks] = 0.0
            p = np.exp(s - s.max(-1, keepdims=True))
            o = (p / p.sum(-1, keepdims=True)) @ vh
            o[:ks] = 0.0
            out[b, :, h * 256:(h + 1) * 256] = o
    return out


def linear(x, w, f64=False):
    """Bias-free Linear, f32 accumulation, the bf16 output MLX stores. f64: the same product accumulated in f64 - a change of
    accumulation error only, used to measure how far the replay moves against itself."""
    if f64:
        return bf16((np.asarray(x, np.float64) @ np.asarray(w, np.float64).T).astype(F32))
    return bf16(np.asarray(x, F32) @ np.asarray(w, F32).T)


def key_start_of(mask):
    """Left-padded masks 0..0 1..1 only; None for any other form."""
    out = []
    for row in np.asarray(mask):
        ones = int((row == 1).sum())
        if ones < 1 or not np.isin(row, (0, 1)).all() or not (row[len(row) - ones:] == 1).all():
            return None
        out.append(len(row) - ones)
    return np.array(out, np.int32)


def layer_key(i, name):
    return f"model.layers.{i}.{name}.weight"


def synth_weights(cfg, seed, embed_std=0.4):
    """bf16-representable f32 arrays under the reference's module keys; norm weights are the stored w of the 1 + w form.
    Embedding rows are N(0, 0.4^2): after the sqrt(hidden) scaling the residual stream (RMS 8 at hidden 384) is several times a
    sublayer's unit-RMS post-norm output, the conditioning the embedding scaling gives the trained model. With a unit-RMS stream
    every sublayer rewrites half of the stream, and the 7-layer replay is not reproducible to the 1e-2 stack bound against ITSELF:
    accumulating its own GEMMs in f64 instead of f32 moves hidden state 7 by 1.1e-2 (6e-3 at RMS 8). embed_std = 0.05 gives that
    unit-RMS stream (tests/test_gemma_gpu.py measures the library on it against the replay's own noise floor)."""
    rng = np.random.default_rng(seed)
    H, I, Dq, Dk = cfg.hidden, cfg.intermediate, cfg.heads * 256, cfg.kv_heads * 256

    def mat(o, i):
        return bf16(rng.standard_normal((o, i)).astype(F32) / F32(math.sqrt(i)))

    def vec(n):
        return bf16(rng.standard_normal(n).astype(F32) * F32(0.1))

    w = {"model.embed_tokens.weight": bf16(rng.standard_normal((cfg.vocab, H)).astype(F32) * F32(embed_std)), "model.norm.weight": vec(H)}
    for i in range(cfg.layers):
        w[layer_key(i, "self_attn.q_proj")] = mat(Dq, H)
        w[layer_key(i, "self_attn.k_proj")] = mat(Dk, H)
        w[layer_key(i, "self_attn.v_proj")] = mat(Dk, H)
        w[layer_key(i, "self_attn.o_proj")] = mat(H, Dq)
        w[layer_key(i, "self_attn.q_norm")] = vec(256)
        w[layer_key(i, "self_attn.k_norm")] = vec(256)
        for n in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            w[layer_key(i, n)] = vec(H)
        w[layer_key(i, "mlp.gate_proj")] = mat(I, H)
        w[layer_key(i, "mlp.up_proj")] = mat(I, H)
        w[layer_key(i, "mlp.down_proj")] = mat(H, I)
    return w


def forward(cfg, w, ids, mask, gemm_f64=False):
    """Hidden states [layers+1][B][T][hidden] (f32 holding bf16 values): slot 0 the scaled embedding, slot i+1 the output of layer
    i < L-1, the last slot model.norm of the last layer (Gemma3Model.swift:203-303)."""
    ids = np.asarray(ids)
    lin = (lambda x, wm: linear(x, wm, True)) if gemm_f64 else linear
    B, T = ids.shape
    ks = key_start_of(mask)
    assert ks is not None and T <= cfg.sliding_window
    H, eps = cfg.hidden, cfg.rms_eps
    scale = cfg.query_pre_attn_scalar ** -0.5
    tables = {False: rope_tables(T, cfg.rope_local_base), True: rope_tables(T, cfg.rope_theta)}
    x = embed(ids, w["model.embed_tokens.weight"], H).reshape(B * T, H)
    states = [x]
    for i in range(cfg.layers):
        xn = rms_norm(x, w[layer_key(i, "input_layernorm")], eps)
        cos, sin = tables[is_global(cfg, i)]
        q = qknorm_rope(lin(xn, w[layer_key(i, "self_attn.q_proj")]), w[layer_key(i, "self_attn.q_norm")], cos, sin, T, eps)
        k = qknorm_rope(lin(xn, w[layer_key(i, "self_attn.k_proj")]), w[layer_key(i, "self_attn.k_norm")], cos, sin, T, eps)
        v = lin(xn, w[layer_key(i, "self_attn.v_proj")])
        ao = bf16(attention(q.reshape(B, T, -1), k.reshape(B, T, -1), v.reshape(B, T, -1), cfg.heads, cfg.kv_heads, scale, ks))
        r = lin(ao.reshape(B * T, -1), w[layer_key(i, "self_attn.o_proj")])
        h, xn = norm_residual(r, w[layer_key(i, "post_attention_layernorm")], eps, x, w[layer_key(i, "pre_feedforward_layernorm")])
        gu = np.concatenate([lin(xn, w[layer_key(i, "mlp.gate_proj")]), lin(xn, w[layer_key(i, "mlp.up_proj")])], axis=-1)
        r = lin(geglu(gu), w[layer_key(i, "mlp.down_proj")])
        x, _ = norm_residual(r, w[layer_key(i, "post_feedforward_layernorm")], eps, h)
        states.append(x if i < cfg.layers - 1 else rms_norm(x, w["model.norm.weight"], eps))
    return np.stack(states).reshape(cfg.layers + 1, B, T, H)


# ---- MLX affine quantisation (group 64 along the input dim), as mx.quantize lays it out ----
def quantize(wm, bits):
    """codes [out][in] uint8 (values < 2^bits), scales / biases [out][in/64] as bf16-representable f32. w' = bf16(q * scale + bias)."""
    o, i = wm.shape
    g = np.asarray(wm, F32).reshape(o, i // 64, 64)
    lo, hi = g.min(-1), g.max(-1)
    scale = bf16(np.maximum((hi - lo) / F32(2 ** bits - 1), F32(1e-8)))
    bias = bf16(lo)
    q = np.clip(np.rint((g - bias[..., None]) / scale[..., None]), 0, 2 ** bits - 1).astype(np.uint8)
    return q.reshape(o, i), scale, bias


def dequantize(q, scale, bias):
    o, i = q.shape
    g = q.reshape(o, i // 64, 64).astype(F32)
    return bf16(g * scale[..., None] + bias[..., None]).reshape(o, i)


def mlx_pack(q, bits):
    """uint32 words [out][in*bits/32]: element e of a word sits at bits e*bits .. (low bits first), as mx.quantize packs them."""
    o, i = q.shape
    per = 32 // bits
    words = np.zeros((o, i // per), np.uint32)
    qq = q.reshape(o, i // per, per).astype(np.uint32)
    for e in range(per):
        words |= qq[:, :, e] << np.uint32(e * bits)
    return words


def library_code_bytes(q, bits):
    """This library's code layout (dit.h, LinearW): 8 bits one code per byte; 4 bits two per byte, low nibble first."""
    if bits == 8:
        return q.astype(np.uint8).reshape(-1)
    return (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8).reshape(-1)
