"""Gemma-3 token generation on a KV cache (csrc/gemma_generate.cpp) on gemma_ref's 7-layer model (hidden 384, 2 / 1 heads,
intermediate 768, embed_std 0.4, vocabulary 1000), against the numpy replay (tests/helpers/gemma_decode_ref.py).

Teacher-forced, prefill of 40 tokens and 24 forced steps: model.norm of every step within the project's stack bound (rel-L2 1e-2);
the logits within twice what the replay moves against ITSELF when its GEMMs accumulate in f64 (the rule of
tests/test_gemma_gpu.py::test_unit_rms_stream...). Measured on MI355X: see DESIGN.md 6l."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_decode_ref as dec  # noqa: E402
import gemma_ref as ref  # noqa: E402
from st_writer import write_safetensors  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = ref.Config(hidden=384, layers=7, intermediate=768, heads=2, kv_heads=1, vocab=1000)
T0, STEPS, CAP = 40, 24, 96
DK = TINY.kv_heads * 256


def lib_cfg(ltx, c):
    return ltx.gemma_config(hidden_size=c.hidden, num_hidden_layers=c.layers, intermediate_size=c.intermediate, num_attention_heads=c.heads,
                            head_dim=c.head_dim, num_key_value_heads=c.kv_heads, vocab_size=c.vocab, sliding_window=c.sliding_window,
                            sliding_window_pattern=c.sliding_window_pattern)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def tiny(ltx, tmp_path_factory):
    """A context of its own with the tiny model loaded from one bf16 file, the forced token sequence, and the replay of it - computed
    once, with f32 and with f64 GEMM accumulation."""
    w = ref.synth_weights(TINY, 4, embed_std=0.4)
    path = tmp_path_factory.mktemp("lm") / "tiny.safetensors"
    write_safetensors(path, {k: ("BF16", v.shape, ref.bf16_bits(v)) for k, v in w.items()})
    ctx = ltx.Context(0)
    ctx.gemma_load(path, lib_cfg(ltx, TINY))
    ids = np.random.default_rng(8).integers(0, TINY.vocab, T0 + STEPS).astype(np.int32)
    replay = {}
    for f64 in (False, True):
        cache, state, logits = dec.prefill(TINY, w, ids[:T0], f64)
        states, lgs = [state], [logits]
        for t in ids[T0:]:
            state, logits = dec.step(TINY, w, cache, int(t), f64)
            states.append(state)
            lgs.append(logits)
        replay[f64] = (np.stack(states), np.stack(lgs), cache)
    yield {"ctx": ctx, "w": w, "ids": ids, "replay": replay, "path": path}
    ctx.close()


def test_teacher_forced_states_and_logits(tiny):
    ctx, ids = tiny["ctx"], tiny["ids"]
    want_s, want_l, _ = tiny["replay"][False]
    other_s, other_l, _ = tiny["replay"][True]
    ctx.lm_begin(CAP)
    got_l = [ctx.lm_prefill(ids[:T0], TINY.vocab)]
    got_s = [ref.from_bits(ctx.lm_last_state(TINY.hidden))]
    for t in ids[T0:]:
        got_l.append(ctx.lm_step(int(t), TINY.vocab))
        got_s.append(ref.from_bits(ctx.lm_last_state(TINY.hidden)))
    ctx.lm_end()
    got_s, got_l = np.stack(got_s), np.stack(got_l)
    assert np.isfinite(got_s).all() and np.isfinite(got_l).all()
    assert np.array_equal(ref.bf16(got_l), got_l)  # the f32 logits hold bf16 values
    s_rel = [rel_l2(got_s[i], want_s[i]) for i in range(STEPS + 1)]
    l_rel = [rel_l2(got_l[i], want_l[i]) for i in range(STEPS + 1)]
    s_floor = max(rel_l2(other_s[i], want_s[i]) for i in range(STEPS + 1))
    l_floor = max(rel_l2(other_l[i], want_l[i]) for i in range(STEPS + 1))
    for i in range(STEPS + 1):
        print(f"position {T0 - 1 + i}: state rel-L2 {s_rel[i]:.3e}, logits rel-L2 {l_rel[i]:.3e}")
    print(f"worst state rel-L2 {max(s_rel):.3e} (bound 1e-2; replay with f64 GEMMs against itself {s_floor:.3e})")
    print(f"worst logits rel-L2 {max(l_rel):.3e} (bound 2 x {l_floor:.3e}, the replay with f64 GEMMs against itself)")
    assert max(s_rel) <= 1e-2
    assert max(l_rel) <= 2.0 * l_floor


def test_few_row_gemm_baseline_computes_the_same_step(tiny):
    """Option "lm_gemm" = 1 (the measurement baseline of tools/bench_lm_generate.py): every Linear of the step through the few-row GEMM
    at M = 1 and the GeGLU as its own pass. Another accumulation order, the same bound against the replay."""
    ctx, ids = tiny["ctx"], tiny["ids"]
    want_s, want_l, _ = tiny["replay"][False]
    ctx.lm_begin(CAP)
    ctx.set_option("lm_gemm", 1)
    try:
        ctx.lm_prefill(ids[:T0])
        for i in range(1, 5):
            logits = ctx.lm_step(int(ids[T0 + i - 1]), TINY.vocab)
            state = ref.from_bits(ctx.lm_last_state(TINY.hidden))
            assert rel_l2(state, want_s[i]) <= 1e-2 and np.array_equal(ref.bf16(logits), logits)
    finally:
        ctx.set_option("lm_gemm", 0)
        ctx.lm_end()


def test_prefill_k_cache_equals_the_encoders_k(tiny):
    """Rows 0 .. T-1 of every layer's K cache after the prefill, against the K the encoder computes for the same ids - rebuilt from the
    encoder's hidden states with the existing seams: input norm, the fused q|k projection, q/k norm + RoPE. Bit for bit: the prefill runs
    the encoder's launches and only the row pass's K destination differs."""
    ctx, w, ids = tiny["ctx"], tiny["w"], tiny["ids"][:T0]
    H, Dq = TINY.hidden, TINY.heads * 256
    hid = torch.empty((TINY.layers + 1, 1, T0, H), device="cuda", dtype=torch.bfloat16)
    ctx.gemma_encode_dev(torch.from_numpy(ids[None]).cuda(), torch.ones((1, T0), dtype=torch.int32, device="cuda"), hid)
    ctx.lm_begin(CAP)
    ctx.lm_prefill(ids)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    tables = {}
    for glob, base in ((False, TINY.rope_local_base), (True, TINY.rope_theta)):
        cos, sin = torch.empty((T0, 128), device="cuda"), torch.empty((T0, 128), device="cuda")
        ctx.op_gemma_rope_tables(T0, base, cos, sin)
        tables[glob] = (cos, sin)
    for l in range(TINY.layers):
        xn = torch.empty((T0, H), device="cuda", dtype=torch.bfloat16)
        ctx.op_gemma_norm(hid[l, 0], f32(w[ref.layer_key(l, "input_layernorm")]), h=xn)
        wqk = f32(np.concatenate([w[ref.layer_key(l, "self_attn.q_proj")], w[ref.layer_key(l, "self_attn.k_proj")]])).to(torch.bfloat16)
        qk = torch.empty((T0, Dq + DK), device="cuda", dtype=torch.bfloat16)
        ctx.op_gemm(xn, wqk, out_bf16=qk)
        cos, sin = tables[ref.is_global(TINY, l)]
        ctx.op_gemma_qknorm_rope(qk, f32(w[ref.layer_key(l, "self_attn.q_norm")]), f32(w[ref.layer_key(l, "self_attn.k_norm")]), TINY.heads, TINY.kv_heads,
                                 cos, sin, T0, TINY.rms_eps)
        torch.cuda.synchronize()
        want = qk[:, Dq:].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(ctx.lm_cache_k(l, T0, DK), want), l
    ctx.lm_end()


def host_loop(ctx, ids, max_new, penalty, context, eos=()):
    """The generate loop driven from here through prefill / step, with the numpy penalty + argmax on the returned logits."""
    logits = ctx.lm_prefill(ids, TINY.vocab)
    out = []
    while len(out) < max_new:
        tok = dec.pick(dec.penalize(logits, out, context, penalty))
        if tok in eos:
            break
        out.append(tok)
        if len(out) == max_new:
            break
        logits = ctx.lm_step(tok, TINY.vocab)
    return out


def test_greedy_generate_equals_the_host_driven_loop(tiny, ltx):
    """Token for token, and exactly: both run the same kernels on the same cache; only the pick moves from numpy to lm_pick_kernel."""
    ctx, ids = tiny["ctx"], tiny["ids"][:T0]
    ctx.lm_begin(CAP)
    # on this model the last prompt token's own logit leads by 110: under the default penalty 1.1 greedy repeats it for ever. Penalty 8
    # makes the run move on (the replay's margins between the first and second logit are 4.4, 1.5, 6.8 at the next three picks)
    want = host_loop(ctx, ids, 20, 8.0, 64)
    got = ctx.lm_generate(ids, ltx.lm_params(temperature=0.0, max_new_tokens=20, repetition_penalty=8.0, eos_ids=[]))
    assert list(got) == want and len(want) == 20  # the max_new stop
    print("greedy tokens:", want)
    assert len(set(want[:3])) == 3
    # a stop id: the third token of that run ends the run after two
    stop = ctx.lm_generate(ids, ltx.lm_params(temperature=0.0, max_new_tokens=20, repetition_penalty=8.0, eos_ids=[999, want[2]]))
    assert list(stop) == want[:2]
    assert host_loop(ctx, ids, 20, 8.0, 64, eos=(999, want[2])) == want[:2]
    # the default penalty: the repeating run, still token for token
    assert list(ctx.lm_generate(ids, ltx.lm_params(temperature=0.0, max_new_tokens=6, eos_ids=[]))) == host_loop(ctx, ids, 6, 1.1, 64)
    # a short context and another penalty take the other branch of the window
    assert list(ctx.lm_generate(ids, ltx.lm_params(temperature=0.0, max_new_tokens=12, repetition_penalty=1.6, repetition_context=3, eos_ids=[]))) == \
        host_loop(ctx, ids, 12, 1.6, 3)
    assert len(ctx.lm_generate(ids, ltx.lm_params(temperature=0.0, max_new_tokens=0))) == 0
    ctx.lm_end()


def test_sampled_generate_is_seeded_and_uses_the_host_sampler(tiny, ltx):
    ctx, ids = tiny["ctx"], tiny["ids"][:T0]
    ctx.lm_begin(CAP)
    p = dict(temperature=0.7, top_p=0.95, max_new_tokens=10, eos_ids=[], seed=5)
    a = list(ctx.lm_generate(ids, ltx.lm_params(**p)))
    assert a == list(ctx.lm_generate(ids, ltx.lm_params(**p))) and len(a) == 10
    # the same run driven from here: logits to the host, ltx_lm_sample_host with the step index as the draw
    logits, out = ctx.lm_prefill(ids, TINY.vocab), []
    for i in range(10):
        out.append(ltx.lm_sample_host(logits, generated=out, context=64, penalty=1.1, temperature=0.7, top_p=0.95, seed=5, step=i))
        if i < 9:
            logits = ctx.lm_step(out[-1], TINY.vocab)
    assert out == a
    ctx.lm_end()


def test_second_prefill_resets_the_cache(tiny, ltx):
    ctx, ids = tiny["ctx"], tiny["ids"]
    params = ltx.lm_params(temperature=0.0, max_new_tokens=8, eos_ids=[])
    ctx.lm_begin(CAP)
    fresh = list(ctx.lm_generate(ids[:T0], params))
    ctx.lm_generate(ids[7:T0 + 20], params)        # another, longer prompt through the same session
    again = list(ctx.lm_generate(ids[:T0], params))
    ctx.lm_end()
    ctx.lm_begin(CAP)
    new_session = list(ctx.lm_generate(ids[:T0], params))
    ctx.lm_end()
    assert fresh == again == new_session


def test_refusals_and_memory(tiny, ltx):
    ctx, ids = tiny["ctx"], tiny["ids"]

    def refused(fn, code=2):
        with pytest.raises(ltx.LTXError) as e:
            fn()
        assert e.value.code == code, e.value

    assert ctx.lm_memory_info() == {"cache": 0, "workspace": 0} and ctx.lm_end() == 0
    refused(lambda: ctx.lm_prefill(ids[:T0]))           # no session
    refused(lambda: ctx.lm_step(3))
    refused(lambda: ctx.lm_generate(ids[:T0]))
    refused(lambda: ctx.lm_begin(0))
    free0 = torch.cuda.mem_get_info()[0]
    ctx.lm_begin(CAP)
    info = ctx.lm_memory_info()
    ldvt = (CAP + 63) // 64 * 64
    assert info["cache"] == TINY.layers * DK * 2 * (CAP + ldvt) and info["workspace"] > TINY.vocab * 4
    refused(lambda: ctx.lm_step(3))                     # no prompt yet
    refused(lambda: ctx.lm_prefill(ids[:0]))
    refused(lambda: ctx.lm_prefill(np.arange(CAP + 1) % TINY.vocab))                    # above the capacity
    refused(lambda: ctx.lm_prefill(np.array([1, 2, TINY.vocab])))                       # the host entry checks the ids
    refused(lambda: ctx.lm_generate(ids[:T0], ltx.lm_params(temperature=0.0, max_new_tokens=CAP - T0 + 1)))  # T + max_new > capacity
    short = ltx.lm_params(temperature=0.0)
    short.struct_size = 8
    refused(lambda: ctx.lm_generate(ids[:T0], short))
    ctx.lm_prefill(np.arange(CAP - 1) % TINY.vocab)
    ctx.lm_step(3)                                      # fills the last position
    refused(lambda: ctx.lm_step(3))                     # the cache is full
    assert ctx.lm_end() == info["cache"] + info["workspace"]
    assert ctx.lm_memory_info() == {"cache": 0, "workspace": 0}
    # a prompt longer than the sliding window is refused whatever the capacity
    ctx.lm_begin(TINY.sliding_window + 64)
    refused(lambda: ctx.lm_prefill(np.zeros(TINY.sliding_window + 1, np.int32)))
    refused(lambda: ctx.lm_generate(np.zeros(TINY.sliding_window + 1, np.int32), ltx.lm_params(temperature=0.0, max_new_tokens=4)))
    ctx.lm_end()
    # without a model: modelNotLoaded
    other = ltx.Context(0)
    try:
        refused(lambda: other.lm_begin(CAP), code=1)
        refused(lambda: other.lm_generate(ids[:T0]), code=1)
        refused(lambda: other.lm_end(), code=1)
        refused(lambda: other.lm_memory_info(), code=1)
    finally:
        other.close()
