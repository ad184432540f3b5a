"""CPU tests of the Gemma-3 text encoder's host side: the numpy replay (tests/helpers/gemma_ref.py) against an independent torch f32
composition, the configuration defaults, the layer kinds, the RoPE tables, the MLX packing of quantised weights, and the ABI surface."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ltx_gemma_config_default", "ltx_gemma_load", "ltx_gemma_init_synthetic", "ltx_gemma_unload", "ltx_gemma_memory_info",
               "ltx_gemma_encode_dev", "ltx_gemma_encode", "ltx_text_encode_dev", "ltx_text_encode", "ltx_op_attention_causal", "ltx_op_gemma_norm",
               "ltx_op_gemma_qknorm_rope", "ltx_op_gemma_rope_tables", "ltx_op_geglu", "ltx_op_gemma_embed")


def torch_forward(cfg, w, ids, mask):
    """The same graph composed independently in torch f32, no intermediate rounding: F.scaled_dot_product_attention under an explicit
    causal AND padding mask (additive, the dtype's minimum where masked, as the reference builds it), rotate-half RoPE from f64
    frequencies, F.gelu(approximate="tanh"), gains 1 + w in f32."""
    t = {k: torch.from_numpy(v) for k, v in w.items()}
    B, T = ids.shape
    H, eps = cfg.hidden, cfg.rms_eps

    def norm(x, wk):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + t[wk])

    def rope(x, base):  # x [B, heads, T, 256]
        inv = torch.tensor(base, dtype=torch.float64) ** (-torch.arange(128, dtype=torch.float64) / 128.0)
        ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
        cos, sin = torch.cat([ang.cos(), ang.cos()], -1).float(), torch.cat([ang.sin(), ang.sin()], -1).float()
        rot = torch.cat([-x[..., 128:], x[..., :128]], -1)
        return x * cos + rot * sin

    m = torch.from_numpy(mask).bool()
    allowed = torch.tril(torch.ones(T, T, dtype=torch.bool))[None, None] & m[:, None, None, :]
    add = torch.where(allowed, 0.0, torch.finfo(torch.float32).min)
    x = t["model.embed_tokens.weight"][torch.from_numpy(ids).long()] * torch.tensor(math.sqrt(H)).bfloat16().float()
    states = [x]
    for i in range(cfg.layers):
        k_ = lambda n: ref.layer_key(i, n)  # noqa: E731
        xn = norm(x, k_("input_layernorm"))
        q = (xn @ t[k_("self_attn.q_proj")].T).view(B, T, cfg.heads, 256).transpose(1, 2)
        k = (xn @ t[k_("self_attn.k_proj")].T).view(B, T, cfg.kv_heads, 256).transpose(1, 2)
        v = (xn @ t[k_("self_attn.v_proj")].T).view(B, T, cfg.kv_heads, 256).transpose(1, 2)
        base = cfg.rope_theta if ref.is_global(cfg, i) else cfg.rope_local_base
        q, k = rope(norm(q, k_("self_attn.q_norm")), base), rope(norm(k, k_("self_attn.k_norm")), base)
        rep = cfg.heads // cfg.kv_heads
        o = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), attn_mask=add,
                                           scale=cfg.query_pre_attn_scalar ** -0.5)
        r = o.transpose(1, 2).reshape(B, T, -1) @ t[k_("self_attn.o_proj")].T
        h = x + norm(r, k_("post_attention_layernorm"))
        xn = norm(h, k_("pre_feedforward_layernorm"))
        ff = F.gelu(xn @ t[k_("mlp.gate_proj")].T, approximate="tanh") * (xn @ t[k_("mlp.up_proj")].T)
        x = h + norm(ff @ t[k_("mlp.down_proj")].T, k_("post_feedforward_layernorm"))
        states.append(x if i < cfg.layers - 1 else norm(x, "model.norm.weight"))
    return torch.stack(states).numpy()


def test_replay_matches_an_independent_torch_composition():
    cfg = ref.Config(hidden=384, layers=7, intermediate=768, heads=2, kv_heads=1, vocab=64)  # layer 5 is the global one
    w = ref.synth_weights(cfg, 0)
    rng = np.random.default_rng(0)
    ids = rng.integers(0, cfg.vocab, (2, 40)).astype(np.int32)
    mask = np.ones((2, 40), np.int32)
    mask[1, :13] = 0
    got, want = ref.forward(cfg, w, ids, mask), torch_forward(cfg, w, ids, mask)
    assert got.shape == want.shape == (8, 2, 40, 384) and np.isfinite(got).all() and np.isfinite(want).all()
    for l in range(8):
        for b, p in ((0, 0), (1, 13)):
            rel = np.linalg.norm(got[l, b, p:] - want[l, b, p:]) / np.linalg.norm(want[l, b, p:])
            print(f"hidden state {l}, batch element {b}: rel-L2 {rel:.3e}")
            assert rel <= 1e-2, (l, b, rel)
    assert (got[1:, 1, :13] != want[1:, 1, :13]).any()  # padded rows: zeros from the attention here, a uniform average there


def test_config_defaults_are_gemma3configs(ltx):
    c = ltx.gemma_config()
    got = {f: getattr(c, f) for f, _ in c._fields_}
    want = dict(hidden_size=3840, num_hidden_layers=48, intermediate_size=15360, num_attention_heads=16, head_dim=256, num_key_value_heads=8,
                vocab_size=262208, rms_norm_eps=np.float32(1e-6), rope_theta=1000000.0, rope_local_base_freq=10000.0,
                query_pre_attn_scalar=256.0, sliding_window=1024, sliding_window_pattern=6)  # Gemma3Config.swift:42-60
    assert got == want
    r = ref.Config()
    assert (r.hidden, r.layers, r.intermediate, r.heads, r.head_dim, r.kv_heads, r.vocab) == (3840, 48, 15360, 16, 256, 8, 262208)
    assert (r.rope_theta, r.rope_local_base, r.query_pre_attn_scalar, r.sliding_window, r.sliding_window_pattern) == (1e6, 1e4, 256.0, 1024, 6)
    assert r.query_pre_attn_scalar ** -0.5 == 1.0 / 16.0  # the softmax scale: not 1 / sqrt(head_dim) by construction


def test_global_layers_for_pattern_6_over_48_layers():
    cfg = ref.Config()
    assert [i for i in range(48) if ref.is_global(cfg, i)] == [5, 11, 17, 23, 29, 35, 41, 47]
    small = ref.Config(layers=7)
    assert [ref.is_global(small, i) for i in range(7)] == [False] * 5 + [True, False]


def test_rope_table_values():
    for base in (10000.0, 1000000.0):
        cos, sin = ref.rope_tables(1024, base)
        assert cos.shape == sin.shape == (1024, 128) and cos.dtype == np.float32
        assert np.array_equal(cos[0], np.ones(128, np.float32)) and np.array_equal(sin[0], np.zeros(128, np.float32))
        for p, i in ((1, 0), (1, 64), (7, 127), (1023, 0), (1023, 1), (1023, 127), (500, 32)):
            ang = p * base ** (-i / 128.0)
            assert abs(float(cos[p, i]) - math.cos(ang)) <= 1.2e-7 and abs(float(sin[p, i]) - math.sin(ang)) <= 1.2e-7, (base, p, i)
        # frequency 0 is 1 rad per position for either base; frequency 64 is base^-0.5
        assert abs(float(sin[1, 64]) - math.sin(base ** -0.5)) <= 1.2e-7
    assert not np.array_equal(ref.rope_tables(8, 10000.0)[0], ref.rope_tables(8, 1000000.0)[0])


def test_mlx_packed_words_are_the_librarys_code_bytes():
    """mx.quantize packs 32 / bits codes per uint32, element e at bits e * bits ..; little-endian, that is one code per byte at 8 bits and
    two per byte, low nibble first, at 4: the layout launch_dequant reads (dit.h, LinearW). The loader copies the words as they are."""
    rng = np.random.default_rng(0)
    for bits in (4, 8):
        q = rng.integers(0, 2 ** bits, (6, 128)).astype(np.uint8)
        words = ref.mlx_pack(q, bits)
        assert words.dtype == np.uint32 and words.shape == (6, 128 * bits // 32)
        assert np.array_equal(words.astype("<u4").view(np.uint8).reshape(-1), ref.library_code_bytes(q, bits))
        # and back: the codes of a word, low bits first
        back = np.stack([(words >> np.uint32(e * bits)) & np.uint32(2 ** bits - 1) for e in range(32 // bits)], -1).reshape(6, 128)
        assert np.array_equal(back, q)
    w = ref.bf16(rng.standard_normal((4, 128)))
    for bits, tol in ((4, 0.5), (8, 0.05)):
        q, s, b = ref.quantize(w, bits)
        assert q.max() < 2 ** bits and np.abs(ref.dequantize(q, s, b) - w).max() <= tol


def test_left_padded_masks_only():
    assert list(ref.key_start_of(np.array([[1, 1, 1], [0, 0, 1]]))) == [0, 2]
    for bad in ([[1, 1, 0]], [[0, 0, 0]], [[0, 1, 0]], [[0, 2, 1]]):
        assert ref.key_start_of(np.array(bad)) is None


def test_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltxhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    assert {n for n in declared if n.startswith(("ltx_gemma_", "ltx_text_encode"))} <= set(NEW_ENTRIES)
    assert hasattr(ltx, "gemma_config")
    for attr in ("gemma_load", "gemma_init_synthetic", "gemma_unload", "gemma_memory_info", "gemma_encode_dev", "gemma_encode", "text_encode_dev", "text_encode",
                 "op_attention_causal", "op_gemma_norm", "op_gemma_qknorm_rope", "op_gemma_rope_tables", "op_geglu", "op_gemma_embed"):
        assert hasattr(ltx.Context, attr), attr
    assert ctypes.sizeof(lib_mod.GemmaConfig) == 13 * 4
