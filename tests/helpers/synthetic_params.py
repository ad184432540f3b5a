"""What ``*_init_synthetic(seed=7)`` leaves resident in each of the five transformer-family models at its smallest legal shape, as
one sha256 per parameter key. tests/test_param_table_gpu.py compares it with tests/golden/synthetic_param_digests.json, which
tests/golden/make_golden.py --synthetic-digests records. Two layers is the smallest shape at which a per-block view into a stacked
table or a fused matrix can land on the wrong block; the attention module's two distinct dims are the smallest at which swapped rows /
cols show.

The connector has no export entry point, so its parameters are pinned through what they produce: the bits of one encode of a fixed
input (feature extractor, register replacement, final context). Every connector parameter feeds at least one of the three."""
import hashlib

import numpy as np

import dual_block_ref
import dual_model_ref

SEED = 7
DIT = dict(num_layers=2, num_heads=1, in_channels=64, out_channels=64, caption_channels=64)
CONNECTOR = dict(dim=128, heads=1, layers=2, registers=2, states=2)
ATTN = dict(query_dim=64, context_dim=128, heads=1)
DUAL = dict(num_layers=2, video_heads=1, audio_heads=1)  # Dv = 128, Da = 64, context dims 128 / 64
DUAL_MODEL_CHANNELS = dict(in_channels=64, out_channels=64, audio_in_channels=64, audio_out_channels=64, caption_channels=64)
ATTN_KEYS = tuple(f"{p}.{s}" for p in ("to_q", "to_k", "to_v", "to_out") for s in ("weight", "bias")) + ("q_norm.weight", "k_norm.weight")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dit_cfg(ltx):
    return ltx.default_transformer_config(num_layers=DIT["num_layers"], num_attention_heads=DIT["num_heads"], cross_attention_dim=128,
                                          in_channels=DIT["in_channels"], out_channels=DIT["out_channels"],
                                          caption_channels=DIT["caption_channels"])


def expected_keys(oracle):
    """The parameter keys of each model, from the shape tables the parity tests use (not from the library)."""
    return {
        "dit": sorted(oracle.dit_param_shapes(oracle.DiTConfig(**DIT))),
        "connector": ["encode.after_registers", "encode.context", "encode.feature_extractor"],
        "attn_module": sorted(ATTN_KEYS),
        "dual_blocks": sorted(dual_block_ref.param_shapes(2, 1, 1)),
        "dual_model": sorted(dual_model_ref.param_shapes(2, 1, 1, **DUAL_MODEL_CHANNELS)),
    }


def connector_outputs(ctx, oracle):
    import torch

    c = CONNECTOR
    rng = np.random.default_rng(SEED)
    B, T = 2, 8
    hs = oracle.bf16_round((rng.standard_normal((c["states"], B, T, c["dim"])) * 2.0 + 0.25).astype(np.float32))
    am = np.ones((B, T), np.int32)
    am[0, :3] = 0  # left padding: three positions of sample 0 take the learnable registers
    h = torch.from_numpy(oracle.f32_to_bf16_bits(hs).astype(np.int16)).cuda().view(torch.bfloat16)
    m = torch.from_numpy(am).cuda()
    out = torch.empty((B, T, c["dim"]), device="cuda", dtype=torch.bfloat16)
    nc = torch.empty((B, T, c["dim"] * c["states"]), device="cuda", dtype=torch.bfloat16)
    fe = torch.empty((B, T, c["dim"]), device="cuda", dtype=torch.bfloat16)
    reg = torch.empty((B, T, c["dim"]), device="cuda", dtype=torch.float32)
    ctx.connector_encode_dev(h, m, out, taps=(nc, fe, reg))
    torch.cuda.synchronize()
    return {"encode.feature_extractor": fe.view(torch.int16).cpu().numpy(), "encode.after_registers": reg.cpu().numpy(),
            "encode.context": out.view(torch.int16).cpu().numpy()}


def digests(ltx, oracle, ctx):
    """{model: {key: sha256 of the exported f32 values}} on ``ctx``; leaves every model it loaded unloaded again."""
    keys = expected_keys(oracle)
    d = {}
    ctx.dit_init_synthetic(dit_cfg(ltx), seed=SEED)
    d["dit"] = {k: sha(ctx.dit_export_param(k)) for k in keys["dit"]}
    ctx.dit_unload()
    ctx.connector_init_synthetic(ltx.connector_config(**CONNECTOR), seed=SEED)
    d["connector"] = {k: sha(v) for k, v in connector_outputs(ctx, oracle).items()}
    ctx.connector_unload()
    ctx.attn_module_init_synthetic(0, ATTN["query_dim"], ATTN["context_dim"], heads=ATTN["heads"], seed=SEED)
    d["attn_module"] = {k: sha(ctx.attn_module_export_param(0, k)) for k in keys["attn_module"]}
    ctx.attn_module_unload(0)
    ctx.dual_blocks_init_synthetic(ltx.default_dual_block_config(**DUAL), seed=SEED)
    d["dual_blocks"] = {k: sha(ctx.dual_blocks_export_param(k)) for k in keys["dual_blocks"]}
    ctx.dual_blocks_unload()
    ctx.dual_model_init_synthetic(ltx.default_dual_model_config(**DUAL, **DUAL_MODEL_CHANNELS), seed=SEED)
    d["dual_model"] = {k: sha(ctx.dual_model_export_param(k)) for k in keys["dual_model"]}
    ctx.dual_model_unload()
    return d
