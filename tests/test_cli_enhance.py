"""`ltx-video enhance-prompt` (host/ltx_video_cli.cpp over LTXPipeline::enhancePromptTokens, host/LTXVideo.hpp): Gemma-3 prompt
enhancement on token ids. CPU: validation (exit 64) and the refusal `generate --enhance-prompt` keeps. GPU: on gemma_ref's tiny
checkpoint the subcommand writes the ids ltx_lm_generate returns, greedy and sampled."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402
from st_writer import write_safetensors  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc", "build", "ltx-video")
TINY = ref.Config(hidden=384, layers=7, intermediate=768, heads=2, kv_heads=1, vocab=1000)
TINY_FLAGS = ("--gemma-hidden-size", "384", "--gemma-layers", "7", "--gemma-intermediate-size", "768", "--gemma-heads", "2", "--gemma-kv-heads", "1",
              "--gemma-vocab-size", "1000")


def run(*args):
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


def test_validation_errors(ltx):
    rc, _, err = run("enhance-prompt")
    assert rc == 64 and "--gemma-weights" in err
    rc, _, err = run("enhance-prompt", "--token-ids", "chat.safetensors")
    assert rc == 64 and "--gemma-weights" in err
    rc, _, err = run("enhance-prompt", "--gemma-weights", "a.safetensors,b.safetensors")
    assert rc == 64 and "--token-ids" in err
    rc, _, err = run("enhance-prompt", "--gemma-weights", "a.safetensors", "--token-ids", "c.safetensors", "--max-tokens", "0")
    assert rc == 64 and "--max-tokens" in err
    rc, _, err = run("enhance-prompt", "--gemma-weights", "a.safetensors", "--token-ids", "c.safetensors", "--eos-ids", "1,2,3,4,5,6,7,8,9")
    assert rc == 64 and "--eos-ids" in err
    rc, _, err = run("enhance-prompt", "--gemma-weights", "a.safetensors", "--token-ids", "c.safetensors", "--frobnicate")
    assert rc == 64 and "--frobnicate" in err
    # the flag of `generate` stays refused, names itself, and now points at the subcommand
    rc, _, err = run("generate", "x", "--enhance-prompt")
    assert rc == 64 and "--enhance-prompt" in err and "enhance-prompt subcommand" in err
    rc, out, _ = run("--help")
    assert rc == 0 and "enhance-prompt" in out


def read_ids(ltx, path):
    import ctypes

    shp = (ctypes.c_long * 8)()
    assert ltx.lib.ltx_st_info(os.fsencode(path), b"input_ids", shp) == 2 and shp[0] == 1
    out = np.empty(shp[1], np.int32)
    assert ltx.lib.ltx_st_read(os.fsencode(path), b"input_ids", 2, out.ctypes.data, out.size) == out.size
    return out


@pytest.mark.gpu
def test_subcommand_writes_the_ids_of_lm_generate(ltx, tmp_path):
    w = ref.synth_weights(TINY, 4, embed_std=0.4)
    weights = tmp_path / "tiny.safetensors"
    write_safetensors(weights, {k: ("BF16", v.shape, ref.bf16_bits(v)) for k, v in w.items()})
    ids = np.random.default_rng(8).integers(0, TINY.vocab, 40).astype(np.int32)
    chat = tmp_path / "chat.safetensors"
    write_safetensors(chat, {"input_ids": ("I32", (1, 40), ids[None])})
    ctx = ltx.Context(0)
    try:
        ctx.gemma_load(weights, ltx.gemma_config(hidden_size=384, num_hidden_layers=7, intermediate_size=768, num_attention_heads=2,
                                                 num_key_value_heads=1, vocab_size=1000))
        ctx.lm_begin(40 + 12)
        greedy = ctx.lm_generate(ids, ltx.lm_params(temperature=0.0, max_new_tokens=12, eos_ids=[999]))
        sampled = ctx.lm_generate(ids, ltx.lm_params(max_new_tokens=12, seed=21, eos_ids=[999]))
        ctx.lm_end()
    finally:
        ctx.close()
    out = tmp_path / "ids.safetensors"
    rc, text, err = run("enhance-prompt", "--gemma-weights", str(weights), "--token-ids", str(chat), "--max-tokens", "12", "--temperature", "0",
                        "--eos-ids", "999", "--output", str(out), *TINY_FLAGS)
    assert rc == 0, err
    assert np.array_equal(read_ids(ltx, out), greedy) and f"Generated {len(greedy)} tokens" in text
    rc, _, err = run("enhance-prompt", "--gemma-weights", str(weights), "--token-ids", str(chat), "--max-tokens", "12", "--seed", "21", "--eos-ids", "999",
                     "-o", str(out), *TINY_FLAGS)
    assert rc == 0, err
    assert np.array_equal(read_ids(ltx, out), sampled)
