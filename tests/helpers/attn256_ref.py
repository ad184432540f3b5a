"""CPU references for the causal grouped-query attention kernel at head dim 256 (csrc/attention.hip, attn256_causal_kernel): a float64
softmax over the window key_start[b] <= j <= i, a numpy replay of the kernel's rounding points, and the inputs that
tests/test_attention_causal_d256_stress_gpu.py (GPU) and tests/test_attn256_host.py (the replay and the inputs' conditions, no GPU)
share. Layouts: q [B,T,Hq*256], k / v [B,T,Hkv*256], bf16-valued f32; query head h reads K/V head h // (Hq // Hkv)."""
import numpy as np

from gemma_ref import bf16

F32 = np.float32
F64 = np.float64
HEAD_DIM = 256
SCALE = 1.0 / 16.0  # query_pre_attn_scalar^-0.5 at 256
LOG2E = F32(1.4426950408889634)
KV_TILE = 64
BOUNDS = (2e-2, 1e-2)       # max abs, rel-L2: tests/test_attention_causal_d256_gpu.py
RAMP_BOUNDS = (3e-2, 1e-2)  # the two ramp families, as the head-dim-64 and head-dim-128 files give them


def expected_nh(Hq, Hkv):
    """The kernel instance launch_attention_d256 picks: two query heads per wave when the group size is even, else one."""
    assert Hq % Hkv == 0
    return 2 if (Hq // Hkv) % 2 == 0 else 1


def clamp_key_start(key_start, B, T):
    ks = [0] * B if key_start is None else [int(x) for x in key_start]
    assert len(ks) == B
    return [min(max(x, 0), T) for x in ks]


def attention_f64(q, k, v, Hq, Hkv, scale, key_start=None, widen_lo=0, widen_hi=0):
    """softmax(q k^T * scale) v in float64 over keys key_start[b] <= j <= i; rows i < key_start[b] are zero; key_start is clamped to
    [0, T] as the kernel clamps it. widen_lo / widen_hi: the window of every valid row reaches that many keys further down / up (what
    a mask that is off by one computes)."""
    B, T, _ = q.shape
    group = Hq // Hkv
    out = np.zeros((B, T, Hq * HEAD_DIM), F64)
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    for b, ks in enumerate(clamp_key_start(key_start, B, T)):
        if ks >= T:
            continue
        inside = ((j >= ks - widen_lo) & (j <= i + widen_hi)) | (i < ks)  # padding rows: any finite row, zeroed below
        for h in range(Hq):
            kv = slice((h // group) * HEAD_DIM, (h // group + 1) * HEAD_DIM)
            s = (q[b, :, h * HEAD_DIM:(h + 1) * HEAD_DIM].astype(F64) @ k[b, :, kv].astype(F64).T) * float(scale)
            s = np.where(inside, s, -np.inf)
            s -= s.max(-1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(-1, keepdims=True)
            o = p @ v[b, :, kv].astype(F64)
            o[:ks] = 0
            out[b, :, h * HEAD_DIM:(h + 1) * HEAD_DIM] = o
    return out


def attention_replay(q, k, v, Hq, Hkv, scale, key_start=None):
    """attn256_causal_kernel's rounding points in numpy: the workgroup of query tile x walks the 64-key tiles key_start // 64 .. x (a
    tile of padding rows only is zeros); f32 scores, masked to -inf in the diagonal tile and in a first tile that key_start cuts; f32
    running maximum, 0 in its place while a row has no key; p = exp2(fma(s, c, -m c)) with c = scale * log2(e); P rounded to bf16 and the
    denominator summed from the ROUNDED P; f32 accumulation; one division, O = bf16(o * (1 / l)). Not replayed: the order of the f32
    additions inside an MFMA and across lanes."""
    B, T, _ = q.shape
    group = Hq // Hkv
    c = F32(F32(scale) * LOG2E)
    out = np.zeros((B, T, Hq * HEAD_DIM), F32)
    for b, ks in enumerate(clamp_key_start(key_start, B, T)):
        for h in range(Hq):
            kv = slice((h // group) * HEAD_DIM, (h // group + 1) * HEAD_DIM)
            qh, kh, vh = q[b, :, h * HEAD_DIM:(h + 1) * HEAD_DIM].astype(F32), k[b, :, kv].astype(F32), v[b, :, kv].astype(F32)
            for x in range((T + KV_TILE - 1) // KV_TILE):
                r0, r1 = x * KV_TILE, min(T, (x + 1) * KV_TILE)
                if r0 + KV_TILE - 1 < ks:
                    continue
                rows = np.arange(r0, r1)[:, None]
                m_run = np.full((r1 - r0, 1), -np.inf, F32)
                l_run = np.zeros((r1 - r0, 1), F32)
                o = np.zeros((r1 - r0, HEAD_DIM), F32)
                for t in range(ks // KV_TILE, x + 1):
                    k0, k1 = t * KV_TILE, min(T, (t + 1) * KV_TILE)  # keys past T sit above the diagonal of every stored row
                    s = (qh[r0:r1] @ kh[k0:k1].T).astype(F32)
                    if t == x or k0 < ks:
                        keys = np.arange(k0, k1)[None, :]
                        s = np.where((keys < ks) | (keys > rows), F32(-np.inf), s)
                    m_new = np.maximum(m_run, s.max(-1, keepdims=True))
                    m_use = np.where(np.isneginf(m_new), F32(0), m_new)
                    alpha = np.exp2(((m_run - m_use) * c).astype(F32))
                    nmc = (-m_use * c).astype(F32)
                    p = bf16(np.exp2((s.astype(F64) * float(c) + nmc.astype(F64)).astype(F32)))  # one rounding, as the fma
                    l_run = (l_run * alpha + p.sum(-1, keepdims=True, dtype=F32)).astype(F32)
                    o = (o * alpha + p @ vh[k0:k1]).astype(F32)
                    m_run = m_new
                with np.errstate(divide="ignore"):
                    inv = np.where(rows < ks, F32(0), F32(1) / l_run).astype(F32)
                out[b, r0:r1, h * HEAD_DIM:(h + 1) * HEAD_DIM] = bf16((o * inv).astype(F32))
    return out


def attention_errors(got, want):
    """(max abs, rel-L2) of got against want."""
    d = np.asarray(got, F64) - np.asarray(want, F64)
    return float(np.abs(d).max()), float(np.linalg.norm(d) / np.linalg.norm(want))


# ---------------------------------------------------------------------------------------------------------------
# Online-softmax stress inputs. V is N(0, 1) everywhere.
# ---------------------------------------------------------------------------------------------------------------
STRESS_HEADS = ((2, 1), (1, 1))  # NH = 2 and NH = 1
STRESS_KEY_START = (0, 67)
LATE_T = 448                      # seven key tiles
REFMAX_T, REFMAX_KEY, REFMAX_ROW, REFMAX_ROW_BELOW = 330, 290, 301, 311  # tile 4 = keys 256 .. 319 is both rows' diagonal tile


class StressCase:
    """One launch: bf16-valued f32 q / k / v, the head counts, key_start per batch element and the bounds (max abs, rel-L2)."""

    def __init__(self, name, q, k, v, Hq, Hkv, key_start, bounds):
        self.name, self.Hq, self.Hkv, self.key_start, self.bounds = name, Hq, Hkv, tuple(key_start), bounds
        self.nh = expected_nh(Hq, Hkv)
        self.q, self.k, self.v = bf16(q.astype(F32)), bf16(k.astype(F32)), bf16(v.astype(F32))

    def reference(self, key_start=None):
        return attention_f64(self.q, self.k, self.v, self.Hq, self.Hkv, SCALE, self.key_start if key_start is None else key_start)

    def replay(self, key_start=None):
        return attention_replay(self.q, self.k, self.v, self.Hq, self.Hkv, SCALE, self.key_start if key_start is None else key_start)


def _flatten_every_third_query(q):
    q[:, ::3] *= F32(0.05)


def late_maximum_case(Hq, Hkv):
    """Key magnitudes grow along the keys, so every row's running maximum moves in every tile it walks. Every third query is flat except
    for the direction of the key AT key_start, which every other key is orthogonal to: its score there is 16 against about 0.1
    elsewhere, the maximum settles in the first tile walked and alpha is exactly 1 afterwards - moving and settled columns alternate
    inside the 16 queries of each wave, so the ballot sees mixed alpha."""
    B, T = len(STRESS_KEY_START), LATE_T
    rng = np.random.default_rng(2500 + 10 * Hq + Hkv)
    q = rng.standard_normal((B, T, Hq * HEAD_DIM))
    k = rng.standard_normal((B, T, Hkv * HEAD_DIM)) * np.linspace(0.2, 3.0, T)[None, :, None]
    v = rng.standard_normal((B, T, Hkv * HEAD_DIM))
    _flatten_every_third_query(q)
    group = Hq // Hkv
    for b, ks in enumerate(STRESS_KEY_START):
        for hk in range(Hkv):
            cols = slice(hk * HEAD_DIM, (hk + 1) * HEAD_DIM)
            u = rng.choice([-1.0, 1.0], HEAD_DIM)  # |u|^2 = 256: q = u scores 256 / 16 = 16 on k = u
            kk = k[b, :, cols]
            kk -= np.outer(kk @ u / HEAD_DIM, u)
            kk[ks] = u
            for h in range(hk * group, (hk + 1) * group):
                q[b, ::3, h * HEAD_DIM:(h + 1) * HEAD_DIM] += u
    return StressCase(f"late_maximum-Hq{Hq}-Hkv{Hkv}", q, k, v, Hq, Hkv, STRESS_KEY_START, RAMP_BOUNDS)


def far_scores_case(Hq, Hkv, T, sign):
    """Every q.k near sign * 3584, i.e. every scaled score near sign * 224 (c * s about sign * 323): the unshifted exp2 underflows
    (sign -1) or overflows (+1) f32."""
    B = len(STRESS_KEY_START)
    rng = np.random.default_rng(T * 7 + 10 * Hq + Hkv + (sign > 0))
    k = 1.0 + 0.05 * rng.standard_normal((B, T, Hkv * HEAD_DIM))
    q = sign * 14.0 + 0.05 * rng.standard_normal((B, T, Hq * HEAD_DIM))
    v = rng.standard_normal((B, T, Hkv * HEAD_DIM))
    return StressCase(f"far_{'above' if sign > 0 else 'below'}-Hq{Hq}-Hkv{Hkv}-T{T}", q, k, v, Hq, Hkv, STRESS_KEY_START, BOUNDS)


def reference_maximum_case(Hq, Hkv):
    """Ramp to 6 over 330 keys, every third query flat, and rows 301 and 311 of head 0 with one dominant key, 290, in their diagonal
    tile (k = 4 q: score 4 |q|^2 / 16, about 64). Both batch elements hold the SAME q / k / v. key_start = (0, 290): element 1 masks
    everything below the dominant key and not the key itself, so the two elements must agree on rows 301 and 311 of head 0.
    key_start = (0, 291) (REFMAX_MASKED) masks the dominant key in element 1: row 311 must move."""
    T = REFMAX_T
    rng = np.random.default_rng(2900 + 10 * Hq + Hkv)
    q = rng.standard_normal((1, T, Hq * HEAD_DIM))
    k = rng.standard_normal((1, T, Hkv * HEAD_DIM)) * np.linspace(0.2, 6.0, T)[None, :, None]
    v = rng.standard_normal((1, T, Hkv * HEAD_DIM))
    _flatten_every_third_query(q)
    q[0, REFMAX_ROW_BELOW, :HEAD_DIM] = q[0, REFMAX_ROW, :HEAD_DIM]
    k[0, REFMAX_KEY] = 0
    k[0, REFMAX_KEY, :HEAD_DIM] = q[0, REFMAX_ROW, :HEAD_DIM] * 4.0
    q, k, v = (np.repeat(x, 2, axis=0) for x in (q, k, v))
    return StressCase(f"reference_maximum-Hq{Hq}-Hkv{Hkv}", q, k, v, Hq, Hkv, (0, REFMAX_KEY), RAMP_BOUNDS)


REFMAX_MASKED = (0, REFMAX_KEY + 1)


def _grid(*axes):
    return [()] if not axes else [(a,) + rest for a in axes[0] for rest in _grid(*axes[1:])]


# (builder, arguments) of every stress launch
STRESS_CASES = ([(late_maximum_case, a) for a in STRESS_HEADS]
                + [(far_scores_case, h + a) for h in STRESS_HEADS for a in _grid((64, 256, 330), (-1, 1))]
                + [(reference_maximum_case, a) for a in STRESS_HEADS])


def case_id(case):
    builder, args = case
    return builder.__name__.replace("_case", "") + "-" + "-".join(str(a) for a in args)


_built = {}


def build(case):
    """The case's inputs, built once and left unchanged."""
    if case not in _built:
        _built[case] = case[0](*case[1])
    return _built[case]


# the repeatability screen: (B, Hq, Hkv, T, key_start) - six tiles, the last ragged, so both ring stages are reused
REPEAT_SHAPES = ((2, 4, 2, 330, (0, 67)), (1, 3, 1, 330, (129,)))


def repeat_cases(shape):
    """The two inputs the screen launches alternately."""
    B, Hq, Hkv, T, key_start = shape
    assert B == len(key_start)
    return [random_case(Hq, Hkv, T, key_start, seed=100 + n + Hq) for n in range(2)]


def random_case(Hq, Hkv, T, key_start, seed):
    """N(0, 1) keys and values, queries at twice that: q.k / 16 ~ N(0, 2^2), a softmax with a few dominant keys."""
    B = len(key_start)
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, T, Hq * HEAD_DIM)) * 2.0
    k = rng.standard_normal((B, T, Hkv * HEAD_DIM))
    v = rng.standard_normal((B, T, Hkv * HEAD_DIM))
    return StressCase(f"random-Hq{Hq}-Hkv{Hkv}-T{T}", q, k, v, Hq, Hkv, key_start, BOUNDS)


# ---------------------------------------------------------------------------------------------------------------
# Lure sweep: every row's output is ONE value row, bit for bit, unless the mask or the head mapping is off by one.
# Keys are rows of the 256 x 256 Sylvester Hadamard matrix Hm: k_j = (-1)^(j >> 8) * Hm[(j & 255) ^ r], r = 0 for K/V head 0 of batch
# element 0 and another constant per (batch element, K/V head) - Hm[a] * Hm[r] = Hm[a ^ r], so every head's keys are the same
# orthogonal family in another order and a query aimed at one head's key finds another key in any other head. Two keys with
# j mod 256 different are orthogonal; key j +- 256 is minus key j. Row i of query head h is 8 k_tgt + 16 k_lure (entries +-8, +-24, exact
# in bf16): at scale 1/16 the target scores 128, the lure - one key OUTSIDE the window - 256, the target's twin -128, the lure's twin
# -256, every other key 0. The target's P is exactly 1 and every other in-window P rounds to 0 (128 * log2(e) = 184.7 below it).
# ---------------------------------------------------------------------------------------------------------------
LURES = ("upper", "lower")                 # key i + 1 (absent for the last row); key key_start - 1 (absent at key_start = 0)
TARGETS = ("diagonal", "first", "spread")  # key i; key key_start; another key of the window per head
LURE_HEADS = ((1, 1), (2, 1), (3, 1), (3, 3), (4, 1), (4, 2), (6, 2), (6, 3))
LURE_T = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 257)
LURE_KEY_STARTS = (0, 1, 15, 16, 63, 64, 65, 127, 128)
LURE_VARIANTS = (("upper", "diagonal"), ("lower", "first"), ("upper", "spread"), ("lower", "spread"))


def hadamard256():
    h = np.ones((1, 1), F32)
    for _ in range(8):
        h = np.block([[h, h], [h, -h]])
    return h


def key_order(b, hk):
    return (73 * hk + 29 * b) & 255


def lure_keys(B, Hkv, T):
    hm = hadamard256()
    j = np.arange(T)
    sign = np.where((j >> 8) & 1, F32(-1), F32(1))[:, None]
    k = np.empty((B, T, Hkv * HEAD_DIM), F32)
    for b in range(B):
        for hk in range(Hkv):
            k[b, :, hk * HEAD_DIM:(hk + 1) * HEAD_DIM] = sign * hm[(j & 255) ^ key_order(b, hk)]
    return k


def lure_target(target, h, i, ks):
    if target == "diagonal":
        return i
    if target == "first":
        return ks
    return ks + ((i - ks) * (7 + 2 * h) + 3) % (i - ks + 1)


class LureCase:
    """q, k, v, tgt / lure [B,Hq,T] (-1: none - a padding row has no target, a row may have no lure) and the expected output."""

    def __init__(self, Hq, Hkv, T, key_start, lure, target):
        B = len(key_start)
        self.Hq, self.Hkv, self.T, self.key_start, self.nh = Hq, Hkv, T, tuple(key_start), expected_nh(Hq, Hkv)
        group = Hq // Hkv
        rng = np.random.default_rng(1000 * T + 10 * Hq + Hkv + sum(key_start))
        self.k = lure_keys(B, Hkv, T)
        self.v = rng.integers(-8, 9, (B, T, Hkv * HEAD_DIM)).astype(F32)
        self.q = np.empty((B, T, Hq * HEAD_DIM), F32)
        self.tgt = np.full((B, Hq, T), -1)
        self.lure = np.full((B, Hq, T), -1)
        self.expected = np.zeros((B, T, Hq * HEAD_DIM), F32)
        for b, ks in enumerate(key_start):
            for h in range(Hq):
                kv = slice((h // group) * HEAD_DIM, (h // group + 1) * HEAD_DIM)
                for i in range(T):
                    row = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
                    if i < ks:  # a padding row: its output is zeros whatever it asks for
                        self.q[b, i, row] = 8 * self.k[b, i, kv]
                        continue
                    t = lure_target(target, h, i, ks)
                    lu = i + 1 if lure == "upper" else ks - 1
                    if lu < 0 or lu >= T or (lu - t) % 256 == 0:  # no such key, or the target's twin: q would be -8 k_tgt
                        lu = -1
                    self.tgt[b, h, i], self.lure[b, h, i] = t, lu
                    self.q[b, i, row] = 8 * self.k[b, t, kv] + (16 * self.k[b, lu, kv] if lu >= 0 else 0)
                    self.expected[b, i, row] = self.v[b, t, kv]

    def lured_output(self):
        """What a window one key too wide on the lure's side gives in rows that have a lure: the lure's value row."""
        group = self.Hq // self.Hkv
        out = self.expected.copy()
        for b, h, i in zip(*np.nonzero(self.lure >= 0)):
            kv = slice((h // group) * HEAD_DIM, (h // group + 1) * HEAD_DIM)
            out[b, i, h * HEAD_DIM:(h + 1) * HEAD_DIM] = self.v[b, self.lure[b, h, i], kv]
        return out


def _lure_grid():
    """About 150 launches: every T with every key_start of LURE_KEY_STARTS + (T - 1) that is <= T - 1, paired into B = 2 launches from
    the two ends of the list (an odd one out runs at B = 1); every pair under the four LURE_VARIANTS; the head pairs rotate so that
    every variant meets every head pair."""
    cases, n = [], 0
    for T in LURE_T:
        c = sorted({x for x in LURE_KEY_STARTS + (T - 1,) if x <= T - 1})
        pairs = [(c[i], c[-1 - i]) for i in range(len(c) // 2)] + ([(c[len(c) // 2],)] if len(c) % 2 else [])
        for ks in pairs:
            for vi, (lure, target) in enumerate(LURE_VARIANTS):
                Hq, Hkv = LURE_HEADS[(n + 3 * vi) % len(LURE_HEADS)]
                cases.append((Hq, Hkv, T, ks, lure, target))
            n += 1
    return cases


LURE_CASES = _lure_grid()
# the two that also run through the strided entry: NH = 1 with three query heads per K/V head, NH = 2 over two K/V heads
LURE_STRIDED = ((3, 1, 129, (1, 65), "upper", "spread"), (4, 2, 70, (5, 64), "lower", "first"))


def lure_id(c):
    return f"Hq{c[0]}-Hkv{c[1]}-T{c[2]}-ks{'_'.join(map(str, c[3]))}-{c[4]}-{c[5]}"
