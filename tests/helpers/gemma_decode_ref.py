"""CPU replay of Gemma-3 token generation on a KV cache (csrc/gemma_generate.cpp), in numpy, built on gemma_ref: the prefill and
the cached step (Gemma3Model.swift:375-492, Gemma3Attention's cache: path :73-110), the repetition penalty and greedy pick (:438-467),
and this library's own sampler restated independently of the C code.

A step attends ALL cached keys on every layer, sliding ones included: the reference decodes with mask: .none on a KVCacheSimple."""
import numpy as np

import gemma_ref as ref

F32 = np.float32


class Cache:
    """Per layer: the K rows after q/k norm + RoPE and the V rows, one per position."""

    def __init__(self, layers):
        self.k = [None] * layers
        self.v = [None] * layers
        self.len = 0


def _attend(q, k, v, Hq, Hkv, scale, first_pos):
    """Row i of q (position first_pos + i) against keys 0 .. first_pos + i; f32 softmax on the given values, not rounded."""
    n = q.shape[0]
    g = Hq // Hkv
    out = np.zeros((n, Hq * 256), F32)
    for i in range(n):
        nk = first_pos + i + 1
        for h in range(Hq):
            kh = k[:nk, (h // g) * 256:(h // g + 1) * 256].astype(F32)
            vh = v[:nk, (h // g) * 256:(h // g + 1) * 256].astype(F32)
            s = (kh @ q[i, h * 256:(h + 1) * 256].astype(F32)) * F32(scale)
            p = np.exp(s - s.max())
            out[i, h * 256:(h + 1) * 256] = (p / p.sum()) @ vh
    return out


def _rows(cfg, w, cache, ids, gemm_f64=False):
    """The new rows `ids` at positions cache.len ..: appends their K / V to the cache, returns model.norm of the LAST row [hidden]."""
    lin = (lambda x, wm: ref.linear(x, wm, True)) if gemm_f64 else ref.linear
    ids = np.asarray(ids).reshape(-1)
    n, p0 = len(ids), cache.len
    H, eps = cfg.hidden, cfg.rms_eps
    scale = cfg.query_pre_attn_scalar ** -0.5
    tables = {False: ref.rope_tables(p0 + n, cfg.rope_local_base), True: ref.rope_tables(p0 + n, cfg.rope_theta)}
    x = ref.embed(ids, w["model.embed_tokens.weight"], H)
    for i in range(cfg.layers):
        xn = ref.rms_norm(x, w[ref.layer_key(i, "input_layernorm")], eps)
        cos, sin = (t[p0:] for t in tables[ref.is_global(cfg, i)])
        q = ref.qknorm_rope(lin(xn, w[ref.layer_key(i, "self_attn.q_proj")]), w[ref.layer_key(i, "self_attn.q_norm")], cos, sin, n, eps)
        k = ref.qknorm_rope(lin(xn, w[ref.layer_key(i, "self_attn.k_proj")]), w[ref.layer_key(i, "self_attn.k_norm")], cos, sin, n, eps)
        v = lin(xn, w[ref.layer_key(i, "self_attn.v_proj")])
        cache.k[i] = k if cache.k[i] is None else np.concatenate([cache.k[i], k])
        cache.v[i] = v if cache.v[i] is None else np.concatenate([cache.v[i], v])
        ao = ref.bf16(_attend(q, cache.k[i], cache.v[i], cfg.heads, cfg.kv_heads, scale, p0))
        r = lin(ao, w[ref.layer_key(i, "self_attn.o_proj")])
        h, xn = ref.norm_residual(r, w[ref.layer_key(i, "post_attention_layernorm")], eps, x, w[ref.layer_key(i, "pre_feedforward_layernorm")])
        gu = np.concatenate([lin(xn, w[ref.layer_key(i, "mlp.gate_proj")]), lin(xn, w[ref.layer_key(i, "mlp.up_proj")])], axis=-1)
        r = lin(ref.geglu(gu), w[ref.layer_key(i, "mlp.down_proj")])
        x, _ = ref.norm_residual(r, w[ref.layer_key(i, "post_feedforward_layernorm")], eps, h)
    cache.len = p0 + n
    return ref.rms_norm(x[-1], w["model.norm.weight"], eps)


def logits_of(w, state, gemm_f64=False):
    """The tied embedding as lm_head: a bf16 array (asLinear on bf16 operands), held as f32."""
    return ref.linear(state[None], w["model.embed_tokens.weight"], gemm_f64)[0]


def prefill(cfg, w, ids, gemm_f64=False):
    """-> (cache, model.norm of the last row [hidden], its logits [vocab])."""
    assert len(ids) <= cfg.sliding_window
    cache = Cache(cfg.layers)
    state = _rows(cfg, w, cache, ids, gemm_f64)
    return cache, state, logits_of(w, state, gemm_f64)


def step(cfg, w, cache, token, gemm_f64=False):
    """One token at position cache.len -> (model.norm [hidden], logits [vocab])."""
    state = _rows(cfg, w, cache, [token], gemm_f64)
    return state, logits_of(w, state, gemm_f64)


def forced_run(cfg, w, ids, n_prefill, gemm_f64=False):
    """Prefill ids[:n_prefill], then one forced step per remaining id -> (states [n][hidden], logits [n][vocab], cache) with
    n = len(ids) - n_prefill + 1: entry i belongs to position n_prefill - 1 + i."""
    cache, state, logits = prefill(cfg, w, ids[:n_prefill], gemm_f64)
    states, lgs = [state], [logits]
    for t in ids[n_prefill:]:
        state, logits = step(cfg, w, cache, int(t), gemm_f64)
        states.append(state)
        lgs.append(logits)
    return np.stack(states), np.stack(lgs), cache


# ---- penalty, pick, sampler ----
def penalize(logits, generated, context, penalty):
    """A penalised copy: every DISTINCT id among the last min(context, len(generated)) generated tokens, l > 0 ? l / p : l * p in f32."""
    out = np.array(logits, F32)
    n = min(context, len(generated))
    if penalty == 1.0 or n == 0:
        return out
    for t in sorted(set(int(t) for t in generated[len(generated) - n:])):
        if 0 <= t < len(out):
            out[t] = out[t] / F32(penalty) if out[t] > 0 else out[t] * F32(penalty)
    return out


def pick(logits):
    """argmax, ties to the lowest index."""
    return int(np.argmax(logits))


def uniform(ltx, seed, step_index):
    """(w >> 8) * 2^-24, w = word 0 of threefry2x32(mlx_draw_key(seed, step), {0, 0})."""
    w0 = int(ltx.threefry2x32(ltx.mlx_draw_key(seed, step_index), [0, 0])[0])
    return (w0 >> 8) / 16777216.0


def nucleus(logits, temperature, top_p):
    """-> (ids in decreasing probability, ties to the lower id; their f64 weights e^(l/t - max)): the fewest whose mass reaches top_p."""
    z = np.asarray(logits, np.float64) / np.float64(F32(temperature))
    w = np.exp(z - z.max())
    total = 0.0
    for x in w:  # index order, as the library sums
        total += x
    order = np.lexsort((np.arange(len(w)), -w))
    cum = np.cumsum(w[order])
    reach = np.nonzero(cum >= np.float64(F32(top_p)) * total)[0]
    n = int(reach[0]) + 1 if len(reach) else len(w)
    return order[:n], w[order[:n]]


def sample(logits, generated, context, penalty, temperature, top_p, u):
    l = penalize(logits, generated, context, penalty)
    if temperature <= 0:
        return pick(l)
    ids, w = nucleus(l, temperature, top_p)
    cum = np.cumsum(w)
    hit = np.nonzero(cum > u * cum[-1])[0]
    return int(ids[hit[0]] if len(hit) else ids[-1])
