"""The Gemma-3 text encoder (csrc/gemma.cpp) against the numpy replay (tests/helpers/gemma_ref.py): every hidden state on valid rows
within rel-L2 1e-2 (the project's stack bound) and finite; loading from safetensors shards (bf16 with the language_model. prefix, and
MLX 4-bit packed Linears); the rejections; ltx_text_encode_dev against its two halves; the 48-layer model's shape and memory."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402
from st_writer import write_safetensors  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ref.Config(hidden=384, layers=7, intermediate=768, heads=2, kv_heads=1, vocab=512)  # layer 5 global, layer 6 sliding again
WIDE = ref.Config(layers=1, vocab=512)                                                      # 3840 / 16 / 8 / 15360
B, T, PAD = 2, 128, (0, 67)


def lib_cfg(ltx, c):
    return ltx.gemma_config(hidden_size=c.hidden, num_hidden_layers=c.layers, intermediate_size=c.intermediate, num_attention_heads=c.heads,
                            head_dim=c.head_dim, num_key_value_heads=c.kv_heads, vocab_size=c.vocab, sliding_window=c.sliding_window,
                            sliding_window_pattern=c.sliding_window_pattern)


def bf16_file(weights, prefix=""):
    return {prefix + k: ("BF16", v.shape, ref.bf16_bits(v)) for k, v in weights.items()}


def inputs(cfg, seed=0, batch=B, pads=PAD):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cfg.vocab, (batch, T)).astype(np.int32)
    mask = np.ones((batch, T), np.int32)
    for b, p in enumerate(pads):
        mask[b, :p] = 0
    return ids, mask


def encode(ctx, cfg, ids, mask):
    hid = torch.empty((cfg.layers + 1,) + ids.shape + (cfg.hidden,), device="cuda", dtype=torch.bfloat16)
    ctx.gemma_encode_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), hid)
    torch.cuda.synchronize()
    return hid


@pytest.fixture(scope="module")
def small(gpu_ctx, ltx, tmp_path_factory):
    """The small model loaded once from two bf16 shards with the language_model. prefix (plus an lm_head the loader must ignore), its
    weights, one encode and the replay of it."""
    w = ref.synth_weights(SMALL, 1)
    d = tmp_path_factory.mktemp("gemma")
    keys = sorted(w)
    shard1 = bf16_file({k: w[k] for k in keys[::2]}, "language_model.")
    shard2 = bf16_file({k: w[k] for k in keys[1::2]}, "language_model.")
    shard2["language_model.lm_head.weight"] = ("BF16", (4, 4), np.zeros((4, 4), np.uint16))
    write_safetensors(d / "a.safetensors", shard1)
    write_safetensors(d / "b.safetensors", shard2)
    gpu_ctx.gemma_load([d / "a.safetensors", d / "b.safetensors"], lib_cfg(ltx, SMALL))
    ids, mask = inputs(SMALL)
    got = encode(gpu_ctx, SMALL, ids, mask)
    want = ref.forward(SMALL, w, ids, mask)
    yield {"w": w, "dir": d, "ids": ids, "mask": mask, "got": got, "want": want}
    gpu_ctx.gemma_unload()


def check_states(got, want, pads):
    got = got.float().cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for l in range(got.shape[0]):
        for b, p in enumerate(pads):
            g, w = got[l, b, p:], want[l, b, p:]
            rel = np.linalg.norm(g - w) / np.linalg.norm(w)
            print(f"hidden state {l}, batch element {b}: rel-L2 {rel:.3e}")
            worst = max(worst, rel)
    print(f"worst rel-L2 over {got.shape[0]} hidden states: {worst:.3e}")
    assert worst <= 1e-2, worst


def test_small_model_every_hidden_state(small):
    check_states(small["got"], small["want"], PAD)


def test_slot_0_is_the_scaled_embedding_bit_for_bit(small):
    want = ref.embed(small["ids"], small["w"]["model.embed_tokens.weight"], SMALL.hidden)
    assert np.array_equal(small["got"][0].view(torch.int16).cpu().numpy().view(np.uint16), ref.bf16_bits(want))


def test_the_global_layer_uses_the_other_rope_base(small):
    """Layer 5 of 7 is the global one: a replay that runs every layer on the local base misses the bound from slot 6 on."""
    local_only = ref.Config(**{**SMALL.__dict__, "rope_theta": SMALL.rope_local_base})
    other = ref.forward(local_only, small["w"], small["ids"], small["mask"])
    assert np.array_equal(other[:6], small["want"][:6])
    g = small["got"][6, 0].float().cpu().numpy()
    assert np.linalg.norm(g - other[6, 0]) / np.linalg.norm(other[6, 0]) > 1e-2


def test_unit_rms_stream_stays_inside_the_replays_own_noise(gpu_ctx, ltx, small, tmp_path):
    """The looser-conditioned case, as a figure: embedding rows N(0, 0.05^2), a unit-RMS residual stream that every sublayer rewrites by
    half. There the 1e-2 stack bound says nothing about an implementation - the replay misses it against ITSELF when its own GEMMs
    accumulate in f64 instead of f32 (a change of accumulation error only; measured 1.1e-2 at state 7), and the library measures
    1.29e-2. What is asserted: the library's worst state is within 2 x that noise floor - the library differs from the replay by
    accumulation order AND by the bf16 P of the attention kernel, two perturbations of about that size, which add to sqrt(2) of one."""
    w = ref.synth_weights(SMALL, 1, embed_std=0.05)
    write_safetensors(tmp_path / "unit.safetensors", bf16_file(w))
    ids, mask = small["ids"], small["mask"]
    try:
        gpu_ctx.gemma_load(tmp_path / "unit.safetensors", lib_cfg(ltx, SMALL))
        got = encode(gpu_ctx, SMALL, ids, mask).float().cpu().numpy()
    finally:
        gpu_ctx.gemma_load([small["dir"] / "a.safetensors", small["dir"] / "b.safetensors"], lib_cfg(ltx, SMALL))
    want, other = ref.forward(SMALL, w, ids, mask), ref.forward(SMALL, w, ids, mask, gemm_f64=True)

    def worst(a, b):
        return max(float(np.linalg.norm(a[l, e, p:] - b[l, e, p:]) / np.linalg.norm(b[l, e, p:])) for l in range(a.shape[0]) for e, p in enumerate(PAD))
    lib, floor = worst(got, want), worst(other, want)
    print(f"unit-RMS stream: library vs replay {lib:.3e}, replay (f64 GEMMs) vs replay {floor:.3e}")
    assert np.isfinite(got).all() and lib <= 2.0 * floor, (lib, floor)


def test_full_width_layer(gpu_ctx, ltx, small, tmp_path):
    w = ref.synth_weights(WIDE, 2)
    write_safetensors(tmp_path / "wide.safetensors", bf16_file(w))
    try:
        gpu_ctx.gemma_load(tmp_path / "wide.safetensors", lib_cfg(ltx, WIDE))
        ids, mask = inputs(WIDE, 3)
        check_states(encode(gpu_ctx, WIDE, ids, mask), ref.forward(WIDE, w, ids, mask), PAD)
    finally:
        gpu_ctx.gemma_load([small["dir"] / "a.safetensors", small["dir"] / "b.safetensors"], lib_cfg(ltx, SMALL))


def test_packed_4_bit_and_f32_loads_equal_the_dequantised_model(gpu_ctx, ltx, small, tmp_path):
    """Every Linear and the embedding as MLX 4-bit words + scales + biases (one 8-bit), norms as f32: the hidden states equal, bit for
    bit, those of a model given the de-quantised weights as bf16."""
    w = small["w"]
    packed, plain = {}, {}
    for k, v in w.items():
        if v.ndim == 2:
            bits = 8 if k.endswith("layers.0.mlp.down_proj.weight") else 4
            q, s, b = ref.quantize(v, bits)
            packed[k] = ("U32", (v.shape[0], v.shape[1] * bits // 32), ref.mlx_pack(q, bits))
            packed[k[:-7] + ".scales"] = ("BF16", s.shape, ref.bf16_bits(s))
            packed[k[:-7] + ".biases"] = ("BF16", b.shape, ref.bf16_bits(b))
            plain[k] = ref.dequantize(q, s, b)
        else:
            packed[k] = ("F32", v.shape, v.astype(np.float32))
            plain[k] = v
    write_safetensors(tmp_path / "q4.safetensors", packed)
    write_safetensors(tmp_path / "dq.safetensors", bf16_file(plain))
    try:
        gpu_ctx.gemma_load(tmp_path / "q4.safetensors", lib_cfg(ltx, SMALL))
        a = encode(gpu_ctx, SMALL, small["ids"], small["mask"])
        gpu_ctx.gemma_load(tmp_path / "dq.safetensors", lib_cfg(ltx, SMALL))
        b = encode(gpu_ctx, SMALL, small["ids"], small["mask"])
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert not torch.equal(a.view(torch.int16), small["got"].view(torch.int16))  # the quantisation is visible at all
        # the fixture's load - two shards, language_model. prefix, an lm_head to ignore - against the SAME weights from one unprefixed
        # file: a wrong shard merge or prefix strip cannot pass this
        write_safetensors(tmp_path / "one.safetensors", bf16_file(w))
        gpu_ctx.gemma_load(tmp_path / "one.safetensors", lib_cfg(ltx, SMALL))
        c = encode(gpu_ctx, SMALL, small["ids"], small["mask"])
        assert torch.equal(c.view(torch.int16), small["got"].view(torch.int16))
    finally:
        gpu_ctx.gemma_load([small["dir"] / "a.safetensors", small["dir"] / "b.safetensors"], lib_cfg(ltx, SMALL))
    again = encode(gpu_ctx, SMALL, small["ids"], small["mask"])
    assert torch.equal(again.view(torch.int16), small["got"].view(torch.int16))  # the two-shard bf16 load, repeated, bit for bit


def test_rejections(gpu_ctx, ltx, small, tmp_path):
    ids, mask = small["ids"], small["mask"]
    with pytest.raises(ltx.LTXError, match="not left-padded") as e:  # right-padded
        encode(gpu_ctx, SMALL, ids, np.ascontiguousarray(mask[:, ::-1]))
    assert e.value.case == "invalidConfiguration"
    zero = mask.copy()
    zero[0] = 0
    with pytest.raises(ltx.LTXError, match="batch element 0"):
        encode(gpu_ctx, SMALL, ids, zero)
    hole = mask.copy()
    hole[1, 100] = 0
    with pytest.raises(ltx.LTXError, match="batch element 1"):
        encode(gpu_ctx, SMALL, ids, hole)
    long_ids = np.zeros((1, SMALL.sliding_window + 1), np.int32)
    with pytest.raises(ltx.LTXError, match="exceed the sliding window") as e:
        encode(gpu_ctx, SMALL, long_ids, np.ones_like(long_ids))
    assert e.value.case == "invalidConfiguration"
    with pytest.raises(ltx.LTXError, match="token id 512"):  # the host-pointer entry checks the ids
        gpu_ctx.gemma_encode(np.full((1, 16), 512, np.int32), np.ones((1, 16), np.int32), SMALL.layers, SMALL.hidden)
    # the model is still the one loaded, and still encodes
    assert torch.equal(encode(gpu_ctx, SMALL, ids, mask).view(torch.int16), small["got"].view(torch.int16))
    other = ltx.Context(0)
    try:
        bad = lib_cfg(ltx, SMALL)
        bad.head_dim = 128
        with pytest.raises(ltx.LTXError, match="head_dim 128") as e:
            other.gemma_init_synthetic(bad, 0)
        assert e.value.case == "invalidConfiguration"
        missing = {k: v for k, v in small["w"].items() if k != "model.layers.3.self_attn.k_norm.weight"}
        write_safetensors(tmp_path / "missing.safetensors", bf16_file(missing))
        with pytest.raises(ltx.LTXError, match=r"model\.layers\.3\.self_attn\.k_norm\.weight") as e:
            other.gemma_load(tmp_path / "missing.safetensors", lib_cfg(ltx, SMALL))
        assert e.value.case == "weightLoadingFailed"
        with pytest.raises(ltx.LTXError, match="Gemma text encoder"):
            encode(other, SMALL, ids, mask)
    finally:
        other.close()


def test_host_pointer_twin_equals_the_device_call(gpu_ctx, small):
    got = gpu_ctx.gemma_encode(small["ids"], small["mask"], SMALL.layers, SMALL.hidden)
    assert np.array_equal(got, small["got"].view(torch.int16).cpu().numpy().view(np.uint16))


def test_text_encode_is_the_two_calls_in_turn_and_ignores_padded_ids(gpu_ctx, ltx, small):
    ccfg = ltx.connector_config(dim=SMALL.hidden, heads=3, layers=1, registers=128, states=SMALL.layers + 1)
    gpu_ctx.connector_init_synthetic(ccfg, 5)
    try:
        ids, mask = torch.from_numpy(small["ids"]).cuda(), torch.from_numpy(small["mask"]).cuda()
        two = torch.empty((B, T, SMALL.hidden), device="cuda", dtype=torch.bfloat16)
        gpu_ctx.connector_encode_dev(small["got"], mask, two, None)
        one = torch.empty_like(two)
        om = torch.zeros((B, T), device="cuda", dtype=torch.int32)
        gpu_ctx.text_encode_dev(ids, mask, one, om)
        torch.cuda.synchronize()
        assert torch.equal(one.view(torch.int16), two.view(torch.int16)) and bool((om == 1).all())
        assert torch.isfinite(one.float()).all()
        # other token ids at the padded positions: the connector output keeps every bit
        ids2 = small["ids"].copy()
        ids2[1, :PAD[1]] = (ids2[1, :PAD[1]] + 17) % SMALL.vocab
        other = torch.empty_like(two)
        gpu_ctx.text_encode_dev(torch.from_numpy(ids2).cuda(), mask, other, None)
        torch.cuda.synchronize()
        assert torch.equal(other.view(torch.int16), one.view(torch.int16))
        # the host-pointer twin: the same bits, and out-of-range ids are reported, not clamped
        hc, hm = gpu_ctx.text_encode(small["ids"], small["mask"], SMALL.hidden)
        assert np.array_equal(hc, one.view(torch.int16).cpu().numpy().view(np.uint16)) and (hm == 1).all()
        with pytest.raises(ltx.LTXError, match="token id -1"):
            gpu_ctx.text_encode(np.full((1, 128), -1, np.int32), np.ones((1, 128), np.int32), SMALL.hidden)
    finally:
        gpu_ctx.connector_unload()


def test_synthetic_48_layer_model_at_1024_tokens(ltx):
    """The reference's size: output shape and finiteness, and unload gives the memory back (ltx_gemma_memory_info)."""
    ctx = ltx.Context(0)
    try:
        assert ctx.gemma_memory_info() == {"weights": 0, "workspace": 0}
        cfg = ltx.gemma_config()
        ctx.gemma_init_synthetic(cfg, 7)
        info = ctx.gemma_memory_info()
        assert 23.0e9 < info["weights"] < 24.5e9 and info["workspace"] == 0
        ids = torch.randint(0, cfg.vocab_size, (1, 1024), device="cuda", dtype=torch.int32)
        hid = torch.empty((49, 1, 1024, 3840), device="cuda", dtype=torch.bfloat16)
        ctx.gemma_encode_dev(ids, torch.ones_like(ids), hid)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(hid.float()).all()) and float(hid[48].float().abs().mean()) > 0
        held = ctx.gemma_memory_info()
        assert held["workspace"] > 0
        free_loaded = torch.cuda.mem_get_info()[0]
        ctx.gemma_unload()
        assert ctx.gemma_memory_info() == {"weights": 0, "workspace": 0}
        assert torch.cuda.mem_get_info()[0] - free_loaded >= 0.99 * (held["weights"] + held["workspace"])
    finally:
        ctx.close()
