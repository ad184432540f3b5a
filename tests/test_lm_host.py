"""CPU tests (no GPU) of Gemma-3 token generation: the numpy replay on a KV cache (tests/helpers/gemma_decode_ref.py) against the
full-prefix replay it must agree with; the new ABI entries; the host sampler's known answers against its independent restatement;
the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_decode_ref as dec  # noqa: E402
import gemma_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ref.Config(hidden=384, layers=7, intermediate=768, heads=2, kv_heads=1, vocab=1000)

NEW_ENTRIES = ("ltx_lm_params_default", "ltx_lm_begin", "ltx_lm_end", "ltx_lm_memory_info", "ltx_lm_prefill_dev", "ltx_lm_prefill", "ltx_lm_step_dev",
               "ltx_lm_step", "ltx_lm_last_state", "ltx_lm_cache_k", "ltx_lm_cache_vt", "ltx_lm_generate", "ltx_lm_sample_host", "ltx_op_gemv_bf16",
               "ltx_gemv_bf16_rows_per_workgroup", "ltx_op_attention_decode", "ltx_op_lm_pick")


def test_cached_replay_agrees_with_the_full_prefix_replay():
    """Prefill 12 tokens, then 4 cached steps: after each, model.norm of the newest row equals gemma_ref.forward on the same prefix
    within the stack bound (rel-L2 1e-2). The two differ only in how the attention is summed, so the figure sits near f32 noise."""
    w = ref.synth_weights(TINY, 3)
    ids = np.random.default_rng(0).integers(0, TINY.vocab, 16).astype(np.int32)
    cache, state, logits = dec.prefill(TINY, w, ids[:12])
    assert logits.shape == (TINY.vocab,) and np.array_equal(ref.bf16(logits), logits)
    worst = 0.0
    for n in range(12, 17):
        want = ref.forward(TINY, w, ids[None, :n], np.ones((1, n), np.int32))[-1, 0, -1]
        rel = np.linalg.norm(state - want) / np.linalg.norm(want)
        print(f"prefix of {n}: rel-L2 {rel:.3e}")
        worst = max(worst, rel)
        if n < 16:
            state, logits = dec.step(TINY, w, cache, ids[n])
    assert cache.len == 16 and cache.k[0].shape == (16, 256)
    assert worst <= 1e-2, worst


def test_long_run_bound_sees_a_key_lost_in_the_second_split(monkeypatch):
    """The bound of tests/test_lm_cache_gpu.py::test_long_forced_run_against_the_replay - twice what the replay moves against itself
    when its GEMMs accumulate in f64 - has teeth: the same model (4 / 2 heads, window 48), a 40-token prefill forced to position 140,
    with key 64 (the first of the second split) dropped from every single-row step's attention. The damaged replay must leave the f32
    one by at least twice that bound at some position after 64. Measured: state 8.6e-2 against the bound 1.56e-2."""
    cfg = ref.Config(hidden=384, layers=7, intermediate=768, heads=4, kv_heads=2, vocab=1000, sliding_window=48)
    w = ref.synth_weights(cfg, 4, embed_std=0.4)
    ids = np.random.default_rng(8).integers(0, cfg.vocab, 141).astype(np.int32)
    want_s, want_l, _ = dec.forced_run(cfg, w, ids, 40)
    other_s, other_l, _ = dec.forced_run(cfg, w, ids, 40, True)
    attend = dec._attend

    def without_key_64(q, k, v, Hq, Hkv, scale, first_pos):
        if q.shape[0] == 1 and first_pos >= 64:
            keep = np.arange(first_pos + 1) != 64
            return attend(q, k[:first_pos + 1][keep], v[:first_pos + 1][keep], Hq, Hkv, scale, first_pos - 1)
        return attend(q, k, v, Hq, Hkv, scale, first_pos)

    monkeypatch.setattr(dec, "_attend", without_key_64)
    bad_s, bad_l, _ = dec.forced_run(cfg, w, ids, 40)
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))
    n = len(want_s)
    s_floor = max(rel(other_s[i], want_s[i]) for i in range(n))
    l_floor = max(rel(other_l[i], want_l[i]) for i in range(n))
    assert all(np.array_equal(bad_s[i], want_s[i]) for i in range(64 - 39))  # positions 39 .. 63 hold no key 64 to lose
    s_bad = [rel(bad_s[i], want_s[i]) for i in range(n)]
    l_bad = [rel(bad_l[i], want_l[i]) for i in range(n)]
    first = 65 - 39  # the entry of position 65
    at = first + int(np.argmax(s_bad[first:]))
    print(f"floors: state {s_floor:.3e}, logits {l_floor:.3e}; without key 64: worst state {s_bad[at]:.3e} at position {39 + at}, "
          f"worst logits {max(l_bad[first:]):.3e}; at position 140 state {s_bad[-1]:.3e}, logits {l_bad[-1]:.3e}")
    assert s_bad[at] >= 2.0 * (2.0 * s_floor) and max(l_bad[first:]) >= 2.0 * (2.0 * l_floor)


def test_new_entries_are_declared_exported_and_bound(ltx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltxhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    assert {n for n in declared if n.startswith("ltx_lm_")} <= set(NEW_ENTRIES)
    for attr in ("lm_begin", "lm_end", "lm_memory_info", "lm_prefill_dev", "lm_prefill", "lm_step_dev", "lm_step", "lm_last_state", "lm_cache_k",
                 "lm_cache_vt", "lm_generate", "op_gemv_bf16", "op_attention_decode", "op_lm_pick"):
        assert hasattr(ltx.Context, attr), attr
    assert lib_mod.LmParams._fields_[0][0] == "struct_size" and lib_mod.LmParams.struct_size.offset == 0


def test_params_default_to_the_references(ltx):
    p = ltx.lm_params()
    assert p.struct_size == ctypes.sizeof(p)
    assert (p.max_new_tokens, p.repetition_context, p.n_eos, p.eos_ids[0]) == (512, 64, 1, 1)
    assert (p.temperature, p.top_p, p.repetition_penalty) == tuple(np.float32(x) for x in (0.7, 0.95, 1.1))
    q = ltx.lm_params(temperature=0.0, eos_ids=[5, 6, 7])
    assert q.temperature == 0.0 and q.n_eos == 3 and list(q.eos_ids[:3]) == [5, 6, 7]
    table = {t[0]: t for t in ltx.option_table()}
    assert table["lm_gemm"][1] == 0 and table["lm_gemm"][4] is True  # a numerics switch, off by default


def test_gemv_rows_per_workgroup_rule(ltx):
    assert ltx.gemv_bf16_rows_per_workgroup(262208, 0) == 16 and ltx.gemv_bf16_rows_per_workgroup(16384, 1) == 16
    assert ltx.gemv_bf16_rows_per_workgroup(16383, 0) == 8 and ltx.gemv_bf16_rows_per_workgroup(3840, 0) == 8
    assert ltx.gemv_bf16_rows_per_workgroup(262208, 2) == 8  # GeGLU: two weight rows per output


# ---- the sampler ----
def test_top_p_near_zero_is_the_argmax(ltx):
    rng = np.random.default_rng(1)
    for s in range(20):
        l = rng.standard_normal(300).astype(np.float32) * 3
        assert ltx.lm_sample_host(l.copy(), temperature=0.9, top_p=1e-6, penalty=1.0, seed=s, step=s) == int(np.argmax(l))


def test_top_p_one_draws_the_distribution(ltx):
    """20 000 seeded draws of a 5-token distribution: every frequency within 4 sigma of its probability."""
    l = np.log(np.array([0.4, 0.3, 0.15, 0.1, 0.05])).astype(np.float32)
    p = np.exp(l.astype(np.float64))
    p /= p.sum()
    n = 20000
    counts = np.bincount([ltx.lm_sample_host(l.copy(), temperature=1.0, top_p=1.0, penalty=1.0, seed=11, step=i) for i in range(n)], minlength=5)
    sigma = np.sqrt(n * p * (1 - p))
    print("counts", counts, "expected", n * p, "sigma", sigma)
    assert (np.abs(counts - n * p) <= 4 * sigma).all()


def test_nucleus_cuts_the_tail_and_ties_go_to_the_lower_id(ltx):
    # probabilities 0.4 0.4 0.1 0.1: top_p 0.5 keeps ids {0, 1} (0.4 < 0.5 <= 0.8), never 2 or 3; top_p 0.3 keeps the lower id of the tie
    l = np.log(np.array([0.4, 0.4, 0.1, 0.1])).astype(np.float32)
    l[1] = l[0]
    seen = {ltx.lm_sample_host(l.copy(), temperature=1.0, top_p=0.5, penalty=1.0, seed=2, step=i) for i in range(200)}
    assert seen == {0, 1}
    assert {ltx.lm_sample_host(l.copy(), temperature=1.0, top_p=0.3, penalty=1.0, seed=2, step=i) for i in range(50)} == {0}
    # the same tie at the far end of a vocabulary, and greedy
    big = np.zeros(262208, np.float32)
    big[[7, 262207]] = 5.0
    assert ltx.lm_sample_host(big.copy(), temperature=1.0, top_p=1e-3, penalty=1.0) == 7
    assert ltx.lm_sample_host(big.copy(), temperature=0.0) == 7


def test_penalty_sign_rule_and_distinct_ids(ltx):
    l = np.array([2.0, -2.0, 0.0, 1.5, 3.0, -1.0], np.float32)
    gen = [4, 1, 4, 2, 0]  # id 4 twice: penalised once; context 4 leaves out the oldest entry (the first 4, still covered) ...
    got = l.copy()
    ltx.lm_sample_host(got, generated=gen, context=4, penalty=1.5, temperature=0.0)
    want = l.copy()
    want[4] = np.float32(3.0) / np.float32(1.5)
    want[1] = np.float32(-2.0) * np.float32(1.5)
    want[0] = np.float32(2.0) / np.float32(1.5)
    assert np.array_equal(got, want) and np.array_equal(got, dec.penalize(l, gen, 4, 1.5))
    got = l.copy()  # ... and context 2 reaches ids {2, 0} only
    assert ltx.lm_sample_host(got, generated=gen, context=2, penalty=1.5, temperature=0.0) == 4
    assert np.array_equal(got, dec.penalize(l, gen, 2, 1.5)) and got[4] == 3.0 and got[1] == -2.0
    for args in (dict(generated=[], penalty=1.5), dict(generated=gen, penalty=1.0), dict(generated=gen, context=0, penalty=1.5)):
        got = l.copy()  # nothing generated, p == 1, or an empty window: untouched
        ltx.lm_sample_host(got, temperature=0.0, **args)
        assert np.array_equal(got, l)
    got = l.copy()  # ids outside the vocabulary are passed over
    ltx.lm_sample_host(got, generated=[-1, 6, 100], penalty=2.0, temperature=0.0)
    assert np.array_equal(got, l)


def test_same_seed_same_token_and_the_restatement_agrees(ltx):
    rng = np.random.default_rng(5)
    l = (rng.standard_normal(1000) * 2).astype(np.float32)
    gen = [int(t) for t in rng.integers(0, 1000, 80)]
    toks = []
    for i in range(40):
        a = ltx.lm_sample_host(l.copy(), generated=gen, context=64, penalty=1.1, temperature=0.7, top_p=0.95, seed=9, step=i)
        b = ltx.lm_sample_host(l.copy(), generated=gen, context=64, penalty=1.1, temperature=0.7, top_p=0.95, seed=9, step=i)
        assert a == b == dec.sample(l, gen, 64, 1.1, 0.7, 0.95, dec.uniform(ltx, 9, i)), i
        toks.append(a)
    assert len(set(toks)) > 5  # steps of one seed are different draws
    ids, _ = dec.nucleus(dec.penalize(l, gen, 64, 1.1), 0.7, 0.95)
    assert set(toks) <= set(int(i) for i in ids) and len(ids) < 1000


# ---- refusals that need no device ----
def test_refusals_without_a_device(ltx):
    lib = ltx.lib
    l = np.zeros(8, np.float32)
    tok = ctypes.c_int32()
    ok = lambda **kw: lib.ltx_lm_sample_host(kw.get("logits", l.ctypes.data), kw.get("vocab", 8), None, kw.get("n", 0), 64, kw.get("penalty", 1.1),
                                             kw.get("t", 0.7), kw.get("top_p", 0.95), 0, 0, kw.get("tok", ctypes.byref(tok)))
    assert ok() == 0
    for bad in (dict(logits=None), dict(vocab=0), dict(tok=None), dict(n=3), dict(penalty=0.0), dict(top_p=0.0), dict(top_p=1.5)):
        assert ok(**bad) == 2, bad
    assert ok(top_p=0.0, t=0.0) == 0  # greedy ignores top_p
    # every context entry refuses a null context
    assert lib.ltx_lm_begin(None, 64) == 2 and lib.ltx_lm_end(None, None) == 2 and lib.ltx_lm_memory_info(None, None, None) == 2
    assert lib.ltx_lm_prefill(None, None, 0, None) == 2 and lib.ltx_lm_step(None, 0, None) == 2
    assert lib.ltx_lm_generate(None, None, 0, None, None, None) == 2
    assert lib.ltx_op_gemv_bf16(None, None, None, 0, 1, 1, 8, 0, None, 1, None) == 2
    assert lib.ltx_op_attention_decode(None, None, None, 0, None, 0, 1, 1, 1, 1.0, None) == 2
    assert lib.ltx_op_lm_pick(None, None, 0, None, 0, 0, 1.0, None) == 2
