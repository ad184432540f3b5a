"""CPU references for the head-dim-64 attention work: the RoPE tables of real-valued 1-D positions and LTXAttention at heads x 64 with
separate query / key tables (LTXAttention.swift:160-218, LTXRoPE.swift:375-490,627-655, LTX2Transformer.swift:176-233), composed from the
oracle's primitives (linear, rms_norm, apply_split_rope, sdpa, bf16_round - all generic in the head count) plus a plain numpy
restatement of what the oracle's `attention` lacks: real positions and key tables of their own."""
import math

import numpy as np

import ltx_oracle as oracle

F32 = np.float32
HEAD_DIM = 64
SCALE = 1.0 / math.sqrt(HEAD_DIM)
QUERY_PRESCALE = F32(F32(0.125) * F32(1.4426950408889634))  # (1 / sqrt(64)) * log2(e) in f32
PARAMS = ("to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias", "to_out.weight", "to_out.bias",
          "q_norm.weight", "k_norm.weight")


def audio_positions(T_a, hop=160, rate=16000, scale=4, offset=1):
    """createAudioPositionGrid in f32: seconds of the middle of audio latent frame i."""
    s, o, h, r = F32(scale), F32(offset), F32(hop), F32(rate)
    out = []
    for i in range(T_a):
        fi = F32(i)
        start = max(F32(0), F32(F32(F32(fi * s) + o) - s))
        end = max(F32(0), F32(F32(F32(F32(fi + F32(1)) * s) + o) - s))
        out.append(F32(F32(F32(F32(start + end) / F32(2)) * h) / r))
    return np.array(out, F32)


def video_temporal_positions(F, H, W, fps=24.0):
    return np.ascontiguousarray(oracle.position_grid(F, H, W, fps)[0])


def rope_tables_positions(pos, dim, theta=10000.0, max_pos=20):
    """precomputeFreqsCis, f64 path, one position dimension: cos, sin [T][dim/2] f32 (no padding: dim/2 frequencies)."""
    n = max(1, dim // 2)
    log_start, log_end = math.log(1.0) / math.log(theta), math.log(theta) / math.log(theta)
    idx = [math.pow(theta, log_start + (log_end - log_start) * i / (n - 1) if n > 1 else log_start) * (math.pi / 2.0) for i in range(n)]
    cos = np.empty((len(pos), n), F32)
    sin = np.empty((len(pos), n), F32)
    for t, p in enumerate(pos):
        scaled = (float(F32(p)) / float(max_pos)) * 2.0 - 1.0
        for i in range(n):
            v = idx[i] * scaled
            cos[t, i] = F32(math.cos(v))
            sin[t, i] = F32(math.sin(v))
    return cos, sin


def ulp_distance(a, b):
    """Largest distance in f32 units in the last place between two f32 arrays of one sign pattern (or exact zeros)."""
    ia = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max())


def attention_f32(q, k, v, heads, scale, bias=None):
    """softmax(q k^T * scale + bias) v per head in f32 on [B,T,heads*64] arrays (the oracle's sdpa)."""
    return oracle.sdpa(q.astype(F32), k.astype(F32), v.astype(F32), heads, scale, bias)


def qknorm_rope(x, w, cos, sin, heads, out_scale=1.0, eps=1e-6):
    """q/k RMSNorm across the whole row, split RoPE per 64-wide head, the folded output scale. x [B,T,heads*64] f32."""
    y = oracle.rms_norm(x, w, eps)
    if cos is not None:
        y = oracle.apply_split_rope(y, cos[:x.shape[1]], sin[:x.shape[1]], heads)
    return (y * F32(out_scale)).astype(F32)


def module_forward(w, x, heads, context=None, q_tables=None, k_tables=None, bias=None, kv_bf16=False, eps=1e-6):
    """LTXAttention.callAsFunction at head dim 64. w: name -> array (PARAMS, weights [out,in]); x [B,Tq,Dq] f32; context [B,Tk,Dc]
    (None: self-attention); q_tables / k_tables (cos, sin) [T][heads*32] (k_tables None: `kPe ?? pe`); kv_bf16: the context, K and V
    are bf16 as in the reference's text cross-attention (oracle.attention(kv_bf16=True))."""
    ctx = x if context is None else context
    q = oracle.linear(x, w["to_q.weight"], w["to_q.bias"])
    k = oracle.linear(ctx, w["to_k.weight"], w["to_k.bias"])
    v = oracle.linear(ctx, w["to_v.weight"], w["to_v.bias"])
    if kv_bf16:
        k, v = oracle.bf16_round(k), oracle.bf16_round(v)
    q = oracle.rms_norm(q, w["q_norm.weight"], eps)
    k = oracle.rms_norm(k, w["k_norm.weight"], eps)
    if kv_bf16:
        k = oracle.bf16_round(k)
    if q_tables is not None:
        kt = k_tables if k_tables is not None else q_tables
        q = oracle.apply_split_rope(q, q_tables[0][:q.shape[1]], q_tables[1][:q.shape[1]], heads)
        k = oracle.apply_split_rope(k, kt[0][:k.shape[1]], kt[1][:k.shape[1]], heads)
    o = oracle.sdpa(q, k, v, heads, SCALE, bias)
    return oracle.linear(o, w["to_out.weight"], w["to_out.bias"])


# ---------------------------------------------------------------------------------------------------------------
# The attention kernel on its own: a float64 reference, a replay of the kernel's rounding points, and the stress / soft-bias inputs
# that tests/test_attention_d64_stress_gpu.py (GPU) and tests/test_attn64_host.py (the replay, no GPU) share.
# ---------------------------------------------------------------------------------------------------------------
F64 = np.float64
LOG2E = F32(1.4426950408889634)
LN2 = F32(0.6931471805599453)
KV_TILE = 64
MASKED = F32(-10000.0)


def _heads(x, heads, dtype):
    b, t, hd = x.shape
    return np.ascontiguousarray(x.reshape(b, t, heads, hd // heads).transpose(0, 2, 1, 3), dtype=dtype)


def attention_f64(q, k, v, heads, scale, bias=None):
    """softmax(q k^T * scale + bias) v per head in float64 on [B,T,heads*d] arrays, any head dim; bias [B,Tk] in the scores' units."""
    b, tq, hd = q.shape
    qh, kh, vh = _heads(q, heads, F64), _heads(k, heads, F64), _heads(v, heads, F64)
    out = np.empty((b, tq, hd), F64)
    for bi in range(b):
        s = (qh[bi] @ kh[bi].transpose(0, 2, 1)) * float(scale)
        if bias is not None:
            s += np.asarray(bias[bi], F64)[None, None, :]
        s -= s.max(-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(-1, keepdims=True)
        out[bi] = (p @ vh[bi]).transpose(1, 0, 2).reshape(tq, hd)
    return out


def attention_replay(q, k, v, heads, scale, bias=None):
    """attn64_fwd_kernel's rounding points in numpy, on bf16-valued f32 arrays [B,T,heads*64]: 64-key tiles, f32 scores, f32 running
    maximum and sum, p = exp2(fma(s, c, -m c)) in f32 with c = scale * log2(e) (masked: s = s * scale + bias first, c = log2(e)), the sum
    over the UNROUNDED p, P rounded to bf16 before the PV product, f32 accumulation, O / l rounded to bf16. scale <= 0 is the prescaled
    entry: the launcher runs it with scale = ln 2. Not replayed: the order of the f32 additions inside an MFMA and across lanes."""
    scale = F32(LN2 if scale <= 0 else scale)
    b, tq, hd = q.shape
    tk = k.shape[1]
    qh, kh, vh = _heads(q, heads, F32), _heads(k, heads, F32), _heads(v, heads, F32)
    c = LOG2E if bias is not None else F32(scale * LOG2E)
    out = np.empty((b, tq, hd), F32)
    for bi in range(b):
        m_run = np.full((heads, tq, 1), -np.inf, F32)
        l_run = np.zeros((heads, tq, 1), F32)
        o = np.zeros((heads, tq, hd // heads), F32)
        for k0 in range(0, tk, KV_TILE):
            k1 = min(tk, k0 + KV_TILE)
            s = qh[bi] @ kh[bi, :, k0:k1].transpose(0, 2, 1)
            if bias is not None:
                s = (s * scale + np.asarray(bias[bi, k0:k1], F32)[None, None, :]).astype(F32)
            m_new = np.maximum(m_run, s.max(-1, keepdims=True))
            with np.errstate(invalid="ignore"):
                alpha = np.exp2(((m_run - m_new) * c).astype(F32))
            nmc = (-m_new * c).astype(F32)
            p = np.exp2((s.astype(F64) * float(c) + nmc.astype(F64)).astype(F32))  # one rounding, as the fma
            l_run = (l_run * alpha + p.sum(-1, keepdims=True, dtype=F32)).astype(F32)
            o = (o * alpha + oracle.bf16_round(p) @ vh[bi, :, k0:k1]).astype(F32)
            m_run = m_new
        out[bi] = oracle.bf16_round((o / l_run).astype(F32)).transpose(1, 0, 2).reshape(tq, hd)
    return out


def attention_errors(got, want):
    """(max abs, rel-L2) of got against want."""
    d = np.asarray(got, F64) - np.asarray(want, F64)
    return float(np.abs(d).max()), float(np.linalg.norm(d) / np.linalg.norm(want))


# (B, H, Tq) that reach each instance of the kernel (queries per workgroup) under the launcher's grid-fill rule; every test asserts it
INSTANCE_SHAPES = {64: (2, 2, 200), 128: (2, 32, 200), 256: (2, 32, 300)}
DOMINANT_QUERY, DOMINANT_KEY = 17, 750  # reference-maximum stress: query 17 of head 0, a key of the last tile of 768


def random_mask_bias(rng, B, Tk, fraction=0.3):
    """(1 - m) * -10000 with key 0 kept, the mask of the text cross-attention."""
    m = (rng.random((B, Tk)) >= fraction).astype(F32)
    m[:, 0] = 1
    return ((1 - m) * MASKED).astype(F32)


class StressCase:
    """One launch: bf16-valued f32 q / k / v [B,T,H*64], bias [B,Tk] or None, the scale handed to the entry (0: prescaled Q), the
    scale the reference applies to the q it is given, and the bounds (max abs, rel-L2)."""

    def __init__(self, name, q, k, v, bias, entry_scale, ref_scale, bounds, heads):
        self.name, self.bias, self.entry_scale, self.ref_scale, self.bounds, self.heads = name, bias, entry_scale, ref_scale, bounds, heads
        self.q, self.k, self.v = oracle.bf16_round(q.astype(F32)), oracle.bf16_round(k.astype(F32)), oracle.bf16_round(v.astype(F32))

    def reference(self, bias_factor=1.0):
        bias = None if self.bias is None else self.bias * F32(bias_factor)
        return attention_f64(self.q, self.k, self.v, self.heads, self.ref_scale, bias)

    def replay(self):
        return attention_replay(self.q, self.k, self.v, self.heads, self.entry_scale, self.bias)


def _prescale(q, prescaled):
    """The prescaled entry: Q carries (1/8) log2(e), rounded to bf16 once; the reference runs on that Q with scale ln 2 (the same math)."""
    return (q * QUERY_PRESCALE if prescaled else q), (0.0 if prescaled else SCALE), (float(LN2) if prescaled else SCALE)


def late_maximum_case(instance, masked):
    """Key magnitudes grow with the key index, so the running maximum moves in every one of the 7 tiles; every third query is flat and
    settles in the first tile - moving and settled columns alternate inside each 16-query block of a wave."""
    B, H, Tq = INSTANCE_SHAPES[instance]
    Tk, D = 448, H * 64
    rng = np.random.default_rng(500 + instance + masked)
    q = rng.standard_normal((B, Tq, D)).astype(F32)
    k = rng.standard_normal((B, Tk, D)).astype(F32) * np.linspace(0.2, 3.0, Tk).astype(F32)[None, :, None]
    q[:, ::3] *= F32(0.05)
    v = rng.standard_normal((B, Tk, D)).astype(F32)
    bias = random_mask_bias(rng, B, Tk) if masked else None
    return StressCase(f"late_maximum-{instance}-{'masked' if masked else 'plain'}", q, k, v, bias, SCALE, SCALE, (3e-2, 1e-2), H)


def far_scores_case(instance, masked, Tk, sign, prescaled):
    """Every score near sign * 224 (c * s about sign * 323): the unshifted exp2 underflows (sign -1) or overflows (+1)."""
    B, H, Tq = INSTANCE_SHAPES[instance]
    D = H * 64
    rng = np.random.default_rng(Tk * 7 + instance + 2 * masked + (sign > 0) + 4 * prescaled)
    k = (1.0 + 0.05 * rng.standard_normal((B, Tk, D))).astype(F32)
    q = (sign * 28.0 + 0.05 * rng.standard_normal((B, Tq, D))).astype(F32)
    v = rng.standard_normal((B, Tk, D)).astype(F32)
    bias = random_mask_bias(rng, B, Tk) if masked else None
    q, entry_scale, ref_scale = _prescale(q, prescaled)
    name = f"far_{'above' if sign > 0 else 'below'}-{instance}-{'masked' if masked else 'plain'}-Tk{Tk}-{'prescaled' if prescaled else 'scaled'}"
    return StressCase(name, q, k, v, bias, entry_scale, ref_scale, (2e-2, 1e-2), H)


def reference_maximum_case(instance, masked):
    """Ramp to 6 over 768 keys, every third query flat, and query 17 of head 0 with one dominant key in the last tile (k = 4 q, the
    key's other heads zero). Both batch elements hold the SAME q / k / v; masked: the same random mask too, except that the dominant key
    is masked in element 1 and not in element 0, so the two outputs must differ at that query."""
    B, H, Tq = INSTANCE_SHAPES[instance]
    Tk, D = 768, H * 64
    rng = np.random.default_rng(900 + instance + masked)
    q = rng.standard_normal((1, Tq, D)).astype(F32)
    k = rng.standard_normal((1, Tk, D)).astype(F32) * np.linspace(0.2, 6.0, Tk).astype(F32)[None, :, None]
    q[:, ::3] *= F32(0.05)
    k[0, DOMINANT_KEY] = 0
    k[0, DOMINANT_KEY, :64] = q[0, DOMINANT_QUERY, :64] * F32(4.0)
    v = rng.standard_normal((1, Tk, D)).astype(F32)
    q, k, v = (np.repeat(x, B, axis=0) for x in (q, k, v))
    bias = None
    if masked:
        bias = np.repeat(random_mask_bias(rng, 1, Tk, 0.2), B, axis=0)
        bias[0, DOMINANT_KEY], bias[1, DOMINANT_KEY] = 0, MASKED
    return StressCase(f"reference_maximum-{instance}-{'masked' if masked else 'plain'}", q, k, v, bias, SCALE, SCALE, (3e-2, 1e-2), H)


def soft_bias_case(instance, prescaled, heads=None, head_dim=64):
    """bias ~ U(-4, 4) per key, another draw per batch element, Tk = 330 (ragged): the bias is in the units of q.k * scale."""
    B, H, Tq = INSTANCE_SHAPES[instance]
    H = H if heads is None else heads
    Tk, D = 330, H * head_dim
    rng = np.random.default_rng(1300 + instance + prescaled + head_dim)
    q = rng.standard_normal((B, Tq, D)).astype(F32)
    k = rng.standard_normal((B, Tk, D)).astype(F32)
    v = rng.standard_normal((B, Tk, D)).astype(F32)
    bias = rng.uniform(-4.0, 4.0, (B, Tk)).astype(F32)
    scale = 1.0 / math.sqrt(head_dim)
    if prescaled:
        q, entry_scale, ref_scale = q * F32(F32(scale) * LOG2E), 0.0, float(LN2)
    else:
        entry_scale = ref_scale = scale
    return StressCase(f"soft_bias-{instance}-{'prescaled' if prescaled else 'scaled'}", q, k, v, bias, entry_scale, ref_scale, (2e-2, 1e-2), H)


def _grid(*axes):
    return [()] if not axes else [(a,) + rest for a in axes[0] for rest in _grid(*axes[1:])]


# (builder, arguments) of every stress / soft-bias launch; the ids are the cases' names
STRESS_CASES = ([(late_maximum_case, a) for a in _grid((64, 128, 256), (False, True))]
                + [(far_scores_case, a) for a in _grid((64, 128, 256), (False, True), (64, 256, 330), (-1, 1), (False, True))]
                + [(reference_maximum_case, a) for a in _grid((64, 128, 256), (False, True))])
SOFT_BIAS_CASES = [(soft_bias_case, a) for a in _grid((64, 128, 256), (False, True))]


def case_id(case):
    builder, args = case
    return builder.__name__.replace("_case", "") + "-" + "-".join(str(int(a)) if isinstance(a, bool) else str(a) for a in args)


# Edge sweep: (instance, B, H, Tq) with Tq on and next to a multiple of the instance's queries per workgroup w, and 2w + 17. The
# 128-query instance cannot run Tq <= 128: one workgroup of 256 queries covers those as well, and the grid-fill rule takes the largest
# size that gives 128 workgroups - so its first boundary is 2w = 256 (Tq = 255, 256, 257), beside w + 1 and 2w + 17.
EDGE_SHAPES = [(64, 2, 3, 63), (64, 2, 3, 64), (64, 2, 3, 65), (64, 2, 3, 145),
               (128, 2, 32, 129), (128, 2, 32, 255), (128, 2, 32, 256), (128, 2, 25, 257), (128, 2, 25, 273),
               (256, 2, 64, 255), (256, 2, 64, 256), (256, 2, 64, 257), (256, 2, 64, 529)]
EDGE_TK = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def one_hot_case(rng, B, H, Tq, Tk):
    """q, k, v [B,T,H*64] and sel [B,H,Tq]: k rows are +-1 codes, q = 16 x the selected key's code (score 128 against N(0, 16) for the
    others), v small integers, so O[b, i, head h] = v[b, sel[b,h,i], head h]. Every key of the last (partial) tile, key 0 and key Tk-1
    are selected by some query. Tk < 8: no margin between codes - every key of a head carries the same v row instead."""
    D = H * 64
    sel = rng.integers(0, Tk, (B, H, Tq))
    need = np.unique(np.concatenate([[0, Tk - 1], np.arange(KV_TILE * ((Tk - 1) // KV_TILE), Tk)]))
    sel.reshape(-1)[rng.permutation(sel.size)[:need.size]] = need
    codes = rng.choice([-1.0, 1.0], (B, H, Tk, 64)).astype(F32)
    k = np.ascontiguousarray(codes.transpose(0, 2, 1, 3)).reshape(B, Tk, D)
    q = np.empty((B, Tq, D), F32)
    for b in range(B):
        for h in range(H):
            q[b, :, h * 64:(h + 1) * 64] = codes[b, h][sel[b, h]] * F32(16.0)
    v = rng.integers(-8, 9, (B, Tk, D)).astype(F32)
    if Tk < 8:
        v[:] = v[:, :1]
    return q, k, v, sel


def one_hot_expected(v, sel, H):
    B, _, Tq = sel.shape
    want = np.empty((B, Tq, H * 64), F32)
    for b in range(B):
        for h in range(H):
            want[b, :, h * 64:(h + 1) * 64] = v[b, sel[b, h], h * 64:(h + 1) * 64]
    return want
