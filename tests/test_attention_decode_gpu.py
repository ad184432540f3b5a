"""attn256_decode_kernel + its combine launch (csrc/attention.hip) through ltx_op_attention_decode: one query per head against a KV
cache, keys split 64 per workgroup, P in f32.

Bounds against the float64 softmax are the prefill kernel's: max abs 2e-2, rel-L2 1e-2. With f32 P the measured figures
sit far under them; the output's own rounding to bf16 (2^-9 relative) is what is left. The lure cases are exact: keys are rows of the
256 x 256 Hadamard matrix at chosen positions and zero rows elsewhere, the query is 8 k_tgt, so at scale 1/16 the target scores 128
against 0, every other P underflows to 0 in f32, the combine's factors are exactly 0 or 1 and the output is V[tgt] in every bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402
from attn256_ref import hadamard256  # noqa: E402

pytestmark = pytest.mark.gpu
N_KEYS = (1, 2, 63, 64, 65, 127, 128, 129, 257, 1000, 1536)
HEADS = ((1, 1), (2, 1), (3, 1), (4, 2), (6, 3), (16, 8))
SCALE = 1.0 / 16.0
MAX_ABS, REL_L2 = 2e-2, 1e-2


def dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def softmax_f64(q, k, v, Hq, Hkv, scale):
    """q [Hq*256], k / v [n][Hkv*256] (bf16 values) -> [Hq*256] in float64."""
    g = Hq // Hkv
    out = np.empty(Hq * 256, np.float64)
    for h in range(Hq):
        c = slice((h // g) * 256, (h // g + 1) * 256)
        s = (k[:, c].astype(np.float64) @ q[h * 256:(h + 1) * 256].astype(np.float64)) * scale
        p = np.exp(s - s.max())
        out[h * 256:(h + 1) * 256] = (p / p.sum()) @ v[:, c].astype(np.float64)
    return out


def launch(ctx, q, k, v, Hq, Hkv, n_keys, cap=None, behind=0.0, scale=SCALE):
    """K cache [cap][Hkv*256] and V^T [Hkv*256][roundup(cap, 64)] from the first n_keys rows of k / v; every cache row and column at or
    past n_keys holds `behind`. Returns the output's bf16 bits [Hq*256]."""
    cap = n_keys if cap is None else cap
    ldvt = (cap + 63) // 64 * 64
    kc = np.full((cap, Hkv * 256), behind, np.float32)
    kc[:n_keys] = k[:n_keys]
    vt = np.full((Hkv * 256, ldvt), behind, np.float32)
    vt[:, :n_keys] = v[:n_keys].T
    o = torch.full((Hq * 256,), 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    ctx.op_attention_decode(dev_bf16(q), dev_bf16(kc), dev_bf16(vt), o, Hq, Hkv, n_keys, scale)
    torch.cuda.synchronize()
    return bits(o)


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_every_key_count_against_the_float64_softmax(gpu_ctx, Hq, Hkv):
    """1 key, both sides of one, two and four splits of 64, and the lengths a generation reaches (1000, 1536 = 24 splits)."""
    rng = np.random.default_rng(Hq * 10 + Hkv)
    q = ref.bf16(rng.standard_normal(Hq * 256) * 2.0)
    k = ref.bf16(rng.standard_normal((max(N_KEYS), Hkv * 256)))
    v = ref.bf16(rng.standard_normal((max(N_KEYS), Hkv * 256)))
    worst = [0.0, 0.0]
    for n in N_KEYS:
        got = ref.from_bits(launch(gpu_ctx, q, k, v, Hq, Hkv, n)).astype(np.float64)
        want = softmax_f64(q, k[:n], v[:n], Hq, Hkv, SCALE)
        err, rel = np.abs(got - want).max(), np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"heads {Hq}/{Hkv}, {n} keys: max abs {err:.3e}, rel-L2 {rel:.3e}")
        worst = [max(worst[0], err), max(worst[1], rel)]
        assert np.isfinite(got).all() and err <= MAX_ABS and rel <= REL_L2, (n, err, rel)
    print(f"heads {Hq}/{Hkv}: worst max abs {worst[0]:.3e}, worst rel-L2 {worst[1]:.3e} (bounds {MAX_ABS}, {REL_L2})")


def lure_case(Hq, Hkv, n_keys, targets, seed):
    """Hadamard rows at 40 scattered positions of every K/V head (distinct rows: mutually orthogonal), zeros elsewhere; query head h is
    8 x the key at targets[h]."""
    rng = np.random.default_rng(seed)
    hm = hadamard256()
    k = np.zeros((n_keys, Hkv * 256), np.float32)
    g = Hq // Hkv
    for hk in range(Hkv):
        pos = set(int(p) for p in rng.choice(n_keys, min(40, n_keys), replace=False)) | {targets[h] for h in range(hk * g, hk * g + g)}
        rows = rng.permutation(256)[:len(pos)]
        for p, r in zip(sorted(pos), rows):
            k[p, hk * 256:(hk + 1) * 256] = hm[r]
    q = np.concatenate([8.0 * k[targets[h], (h // g) * 256:(h // g + 1) * 256] for h in range(Hq)])
    v = ref.bf16(rng.standard_normal((n_keys, Hkv * 256)))
    want = np.concatenate([v[targets[h], (h // g) * 256:(h // g + 1) * 256] for h in range(Hq)])
    return q, k, v, want


@pytest.mark.parametrize("Hq,Hkv,n_keys", [(2, 1, 1000), (16, 8, 1536), (3, 1, 257), (1, 1, 65)])
def test_lured_output_is_the_target_row_in_every_bit(gpu_ctx, Hq, Hkv, n_keys):
    """The target in the first split, in the last split, and as the last key, rotated over the query heads."""
    last_split = (n_keys - 1) // 64 * 64
    places = (5, last_split, n_keys - 1)
    for rot in range(3):
        targets = [places[(h + rot) % 3] for h in range(Hq)]
        q, k, v, want = lure_case(Hq, Hkv, n_keys, targets, seed=n_keys + rot)
        f64 = softmax_f64(q, k, v, Hq, Hkv, SCALE)
        assert np.array_equal(ref.bf16_bits(f64.astype(np.float32)), ref.bf16_bits(want))  # the float64 softmax gives the same row
        got = launch(gpu_ctx, q, k, v, Hq, Hkv, n_keys)
        assert np.array_equal(got, ref.bf16_bits(want)), (rot, int((got != ref.bf16_bits(want)).sum()))


@pytest.mark.parametrize("behind", [float("nan"), 1e30])
@pytest.mark.parametrize("Hq,Hkv,n_keys,cap", [(2, 1, 1, 64), (4, 2, 63, 64), (2, 1, 65, 200), (16, 8, 129, 1536), (3, 1, 1000, 1024)])
def test_cache_behind_n_keys_never_reaches_the_result(gpu_ctx, Hq, Hkv, n_keys, cap, behind):
    """Cache rows and V^T columns at or past n_keys (inside the last split's 64 columns, and whole splits behind it) filled with NaN
    and with 1e30: bit-equal to the same launch on a cache that ends at n_keys."""
    rng = np.random.default_rng(n_keys)
    q = ref.bf16(rng.standard_normal(Hq * 256))
    k = ref.bf16(rng.standard_normal((n_keys, Hkv * 256)))
    v = ref.bf16(rng.standard_normal((n_keys, Hkv * 256)))
    clean = launch(gpu_ctx, q, k, v, Hq, Hkv, n_keys)
    dirty = launch(gpu_ctx, q, k, v, Hq, Hkv, n_keys, cap=cap, behind=behind)
    assert np.isfinite(ref.from_bits(clean)).all() and np.array_equal(clean, dirty)


def test_late_maximum_in_the_last_split(gpu_ctx):
    """Scores near 0 everywhere but one key of the last split, 40 above: every earlier split's (m, l, o) is rescaled by e^-40 in the
    combine. Against float64 within the bounds, and the answer is that key's V row to bf16 accuracy."""
    Hq, Hkv, n = 4, 2, 700
    rng = np.random.default_rng(7)
    q = ref.bf16(rng.standard_normal(Hq * 256))
    k = ref.bf16(rng.standard_normal((n, Hkv * 256)) * 0.05)
    v = ref.bf16(rng.standard_normal((n, Hkv * 256)))
    tgt = n - 3
    for hk in range(Hkv):  # the key that both query heads of the group score highly: their normalised sum
        qs = q[2 * hk * 256:(2 * hk + 1) * 256] + q[(2 * hk + 1) * 256:(2 * hk + 2) * 256]
        k[tgt, hk * 256:(hk + 1) * 256] = ref.bf16(qs * (40.0 / SCALE) / (np.linalg.norm(qs) ** 2) * 2.0)
    want = softmax_f64(q, k, v, Hq, Hkv, SCALE)
    got = ref.from_bits(launch(gpu_ctx, q, k, v, Hq, Hkv, n)).astype(np.float64)
    err, rel = np.abs(got - want).max(), np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"late maximum: max abs {err:.3e}, rel-L2 {rel:.3e}")
    assert err <= MAX_ABS and rel <= REL_L2


def test_alternating_inputs_are_repeatable(gpu_ctx):
    """Two inputs, alternating, 50 launches each, through the one split workspace: no launch differs from the first of its input in
    any element (a split read before it was written, or one launch's partials left for the next, would)."""
    Hq, Hkv = 16, 8
    rng = np.random.default_rng(11)
    cases = []
    for n in (1536, 700):
        q = dev_bf16(rng.standard_normal(Hq * 256))
        kc = dev_bf16(rng.standard_normal((1536, Hkv * 256)))
        vt = dev_bf16(rng.standard_normal((Hkv * 256, 1536)))
        cases.append((q, kc, vt, n, torch.empty(Hq * 256, device="cuda", dtype=torch.bfloat16)))
    first = [None, None]
    for it in range(50):
        for i, (q, kc, vt, n, o) in enumerate(cases):
            gpu_ctx.op_attention_decode(q, kc, vt, o, Hq, Hkv, n, SCALE)
            if first[i] is None:
                first[i] = o.clone()
            else:
                assert torch.equal(o, first[i]), (it, i)
    assert not torch.equal(first[0], first[1])


def test_refusals(gpu_ctx, ltx):
    Hq, Hkv, n = 4, 2, 70
    q = dev_bf16(np.zeros(Hq * 256 + 8))
    kc = dev_bf16(np.zeros((n, Hkv * 256 + 8)))
    vt = dev_bf16(np.zeros((Hkv * 256, 128 + 8)))
    o = torch.full((Hq * 256,), 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    ok = dict(q=q, K=kc, Vt=vt, O=o, Hq=Hq, Hkv=Hkv, n_keys=n, scale=SCALE, ldk=Hkv * 256 + 8, ldvt=136)
    gpu_ctx.op_attention_decode(**ok)
    torch.cuda.synchronize()
    o.view(torch.int16).fill_(0x7FC1)
    bad = [dict(q=None), dict(K=None), dict(Vt=None), dict(O=None), dict(Hq=0), dict(Hq=3), dict(Hq=10), dict(Hkv=0), dict(n_keys=0),
           dict(ldk=Hkv * 256 + 4), dict(ldk=Hkv * 256 - 8), dict(ldvt=132), dict(ldvt=120), dict(q=q[1:]), dict(K=kc[0, 1:]), dict(Vt=vt[0, 1:])]
    for b in bad:
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.op_attention_decode(**{**ok, **b})
        assert e.value.code == 2, b
    torch.cuda.synchronize()
    assert (bits(o) == 0x7FC1).all()
