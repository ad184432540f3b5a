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
