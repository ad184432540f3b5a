"""CPU tests behind tests/test_attention_causal_d256_stress_gpu.py: the numpy replay of attn256_causal_kernel's rounding points
(tests/helpers/attn256_ref.py) meets, against the float64 softmax, every numeric bound that file holds the kernel to, on every stress
input used there; every lure case satisfies the conditions that make its expected output exact and its failure certain; the lure grid
covers what it promises; and the strided entry is declared, exported, bound and mirrored."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn256_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_strided_entry_is_declared_exported_bound_and_mirrored(ltx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltxhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    name = "ltx_op_attention_causal_ld"
    assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES
    assert len(lib_mod.SIGNATURES[name][1]) == 20
    assert hasattr(ltx.Context, "op_attention_causal_ld")
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_replay_and_reference_agree_with_a_plain_softmax():
    """The two helpers against a row-by-row softmax written out here, with padding, a ragged T and three query heads per K/V head."""
    c = ref.random_case(3, 1, 70, (5, 0), seed=1)
    want = np.zeros((2, 70, 3 * 256))
    for b, ks in enumerate(c.key_start):
        for h in range(3):
            for i in range(ks, 70):
                s = c.k[b, ks:i + 1, :].astype(np.float64) @ c.q[b, i, h * 256:(h + 1) * 256].astype(np.float64) / 16.0
                p = np.exp(s - s.max())
                want[b, i, h * 256:(h + 1) * 256] = (p / p.sum()) @ c.v[b, ks:i + 1, :].astype(np.float64)
    assert np.abs(c.reference() - want).max() <= 1e-12
    err, rel = ref.attention_errors(c.replay(), want)
    assert err <= ref.BOUNDS[0] and rel <= ref.BOUNDS[1], (err, rel)
    # the clamp: key_start outside [0, T] is 0 or T
    assert np.array_equal(c.reference((-3, 75)), c.reference((0, 70))) and np.array_equal(c.replay((-3, 75)), c.replay((0, 70)))
    assert not c.replay((0, 70))[1].any() and not c.reference((0, 70))[1].any()


@pytest.mark.parametrize("case", ref.STRESS_CASES, ids=ref.case_id)
def test_kernel_replay_meets_the_bounds_on_the_stress_inputs(case):
    c = ref.build(case)
    want, got = c.reference(), c.replay()
    err, rel = ref.attention_errors(got, want)
    print(f"{c.name}: replay max abs {err:.3e} rel-L2 {rel:.3e}")
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert err <= c.bounds[0] and rel <= c.bounds[1], (err, rel)
    for b, ks in enumerate(c.key_start):
        assert not got[b, :ks].any() and not want[b, :ks].any()


@pytest.mark.parametrize("shape", ref.REPEAT_SHAPES, ids=lambda s: f"Hq{s[1]}-Hkv{s[2]}")
def test_kernel_replay_meets_the_bounds_on_the_repeatability_inputs(shape):
    for c in ref.repeat_cases(shape):
        err, rel = ref.attention_errors(c.replay(), c.reference())
        assert err <= c.bounds[0] and rel <= c.bounds[1], (err, rel)


@pytest.mark.parametrize("heads", ref.STRESS_HEADS, ids=lambda h: f"Hq{h[0]}-Hkv{h[1]}")
def test_late_maximum_moves_and_settles_as_it_says(heads):
    """Every row with i % 3 == 0 has its largest score at key_start (the first tile walked) by a wide margin; and in every wave of 16
    queries, some other row's running maximum moves in every later tile below the diagonal one (of which a row may see too few keys
    to promise anything): the ballot sees settled and moving lanes together."""
    c = ref.build((ref.late_maximum_case, heads))
    T = ref.LATE_T
    for b, ks in enumerate(c.key_start):
        s = (c.q[b, :, :256].astype(np.float64) @ c.k[b, :, :256].astype(np.float64).T) / 16.0
        s[np.arange(T)[None, :] > np.arange(T)[:, None]] = -np.inf
        s[:, :ks] = -np.inf
        for i in range(ks, T):
            if i % 3 == 0:
                assert s[i].argmax() == ks and s[i, ks] - np.delete(s[i], ks).max(initial=-np.inf) > 10, (b, i)
        t_lo = ks // 64
        for w0 in range(64 * (t_lo + 2), T, 16):  # waves that walk two full tiles or more before their diagonal tile
            rows = [i for i in range(w0, min(T, w0 + 16)) if i % 3]
            tile_max = np.stack([s[rows, 64 * t:64 * (t + 1)].max(1) for t in range(t_lo, w0 // 64)], 1)
            run = np.maximum.accumulate(tile_max, 1)
            assert (run[:, 1:] > run[:, :-1]).any(0).all(), (b, w0)


@pytest.mark.parametrize("heads", ref.STRESS_HEADS, ids=lambda h: f"Hq{h[0]}-Hkv{h[1]}")
def test_reference_maximum_discriminates(heads):
    """key_start at the dominant key leaves rows 301 and 311 of head 0 where they were, to the bound; key_start one past it moves row
    311 by more than ten times the bound: a kernel that did not mask the dominant key there cannot pass."""
    c = ref.build((ref.reference_maximum_case, heads))
    want = c.reference()
    for row in (ref.REFMAX_ROW, ref.REFMAX_ROW_BELOW):
        assert np.abs(want[0, row, :256] - want[1, row, :256]).max() <= c.bounds[0]
        assert np.abs(want[0, row, :256] - c.v[0, ref.REFMAX_KEY, :256]).max() <= c.bounds[0]
    masked = c.reference(ref.REFMAX_MASKED)
    assert np.array_equal(masked[0], want[0])
    assert np.abs(masked[1, ref.REFMAX_ROW_BELOW, :256] - want[0, ref.REFMAX_ROW_BELOW, :256]).max() > 10 * c.bounds[0]
    err, rel = ref.attention_errors(c.replay(ref.REFMAX_MASKED), masked)
    assert err <= c.bounds[0] and rel <= c.bounds[1], (err, rel)


@pytest.mark.parametrize("case", [(h + (T,) + (s,)) for h in ref.STRESS_HEADS for T in (64, 256, 330) for s in (-1, 1)],
                         ids=lambda a: "-".join(map(str, a)))
def test_far_scores_are_beyond_the_unshifted_exponent(case):
    c = ref.build((ref.far_scores_case, case))
    s = np.einsum("btd,bsd->bts", c.q[:, :, :256].astype(np.float64), c.k[:, :, :256].astype(np.float64)) / 16.0 * case[3]
    assert s.min() > 200 and s.max() < 250  # exp2(log2(e) * 200) and its reciprocal are outside f32


# ---- the lure sweep ----
def test_lure_grid_covers_what_it_promises():
    cases = ref.LURE_CASES
    assert 140 <= len(cases) <= 160 and len(set(cases)) == len(cases)
    for T in ref.LURE_T:
        starts = {s for c in cases if c[2] == T for s in c[3]}
        assert starts == {s for s in ref.LURE_KEY_STARTS + (T - 1,) if s <= T - 1}, T
        assert len(starts) >= 3 or T == 1
    for heads in ref.LURE_HEADS:
        mine = [c for c in cases if c[:2] == heads]
        assert len({(c[2], c[3]) for c in mine}) >= 2 and any(any(c[3]) for c in mine), heads
        assert {(c[4], c[5]) for c in mine} == set(ref.LURE_VARIANTS), heads  # every variant meets every head pair
        assert {len(c[3]) for c in mine} == {1, 2}, heads
    assert {ref.expected_nh(*h) for h in ref.LURE_HEADS} == {1, 2}
    assert all(c[2] <= 330 and c[0] <= 6 and len(c[3]) <= 2 for c in cases)


@pytest.mark.parametrize("case", ref.LURE_CASES + list(ref.LURE_STRIDED), ids=ref.lure_id)
def test_lure_case_satisfies_its_conditions(case):
    """(1) the target is inside the window and the lure is the one key just outside it; (2) the target's score exceeds every other
    in-window score by at least 150 in log2 units, so every other rounded P is exactly 0; (3) no lure is the target's twin; (4) the
    value rows are pairwise distinct, so another key's row cannot pass for the target's; (5) the float64 softmax over the window widened
    by one key on the lure's side returns the lure's row wherever there is a lure - the leak would be caught; (6) the replay gives
    the expected output bit for bit."""
    Hq, Hkv, T, key_start, lure, target = case
    c = ref.LureCase(*case)
    group = Hq // Hkv
    n_lured = 0
    for b, ks in enumerate(key_start):
        for hk in range(Hkv):
            rows = c.v[b, :, hk * 256:(hk + 1) * 256]
            assert len({r.tobytes() for r in rows}) == T
        for h in range(Hq):
            kv = slice((h // group) * 256, (h // group + 1) * 256)
            s = (c.q[b, :, h * 256:(h + 1) * 256].astype(np.float64) @ c.k[b, :, kv].astype(np.float64).T) * ref.SCALE * 1.4426950408889634
            for i in range(T):
                t, lu = c.tgt[b, h, i], c.lure[b, h, i]
                if i < ks:
                    assert t == -1 and lu == -1 and not c.expected[b, i].any()
                    continue
                assert ks <= t <= i
                want_lure = i + 1 if lure == "upper" else ks - 1
                assert lu in (-1, want_lure) and (lu == want_lure or not 0 <= want_lure < T or (want_lure - t) % 256 == 0)
                others = np.delete(s[i, ks:i + 1], t - ks)
                assert s[i, t] - others.max(initial=-np.inf) >= 150
                if lu >= 0:
                    assert (lu - t) % 256 != 0 and s[i, lu] - s[i, t] >= 150
                    n_lured += 1
    assert n_lured > 0 or T == 1 or (lure == "lower" and not any(key_start))
    assert np.array_equal(ref.attention_replay(c.q, c.k, c.v, Hq, Hkv, ref.SCALE, key_start).view(np.uint32), c.expected.view(np.uint32))
    assert np.abs(ref.attention_f64(c.q, c.k, c.v, Hq, Hkv, ref.SCALE, key_start) - c.expected).max() <= 1e-9
    wide = ref.attention_f64(c.q, c.k, c.v, Hq, Hkv, ref.SCALE, key_start, widen_lo=lure == "lower", widen_hi=lure == "upper")
    assert np.abs(wide - c.lured_output()).max() <= 1e-9
    if n_lured:
        assert np.abs(c.lured_output() - c.expected).max() >= 1


def test_lure_targets_meet_every_tile_edge():
    """Over the grid, targets and lures sit on both sides of the 64-key tile boundaries: keys 63, 64, 127 and 128 are each some row's
    target and some row's lure."""
    tgt, lure = set(), set()
    for case in ref.LURE_CASES:
        if case[2] >= 129:
            c = ref.LureCase(*case)
            tgt |= set(np.unique(c.tgt).tolist())
            lure |= set(np.unique(c.lure).tolist())
    assert {63, 64, 127, 128} <= tgt and {63, 64, 127, 128} <= lure
