"""`ltx-video generate` with the Gemma-3 text encoder: --gemma-weights FILE[,FILE...] --token-ids FILE [--negative-token-ids FILE] as an
alternative to --gemma-hidden-states / --embeddings. Argument handling and validation messages, on CPU (nothing is loaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc", "build", "ltx-video")


def run(*args):
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


def test_gemma_flags_pass_the_dry_run(ltx):
    rc, out, err = run("generate", "x", "--dry-run", "--gemma-weights", "a.safetensors,b.safetensors", "--token-ids", "ids.safetensors")
    assert rc == 0, err
    assert "Text encoder: Gemma-3 (2 shard(s))" in out and "negative prompt" not in out
    assert out.strip().endswith("Validation passed (dry run mode)")
    rc, out, err = run("generate", "x", "--dry-run", "--gemma-weights", "a.safetensors", "--token-ids", "ids.safetensors",
                       "--negative-token-ids", "neg.safetensors")
    assert rc == 0, err
    assert "Text encoder: Gemma-3 (1 shard(s)), with a negative prompt" in out


@pytest.mark.parametrize("args,msg", [
    (["--gemma-weights", "a.safetensors"], "--gemma-weights needs --token-ids (the tokenizer is outside this build)"),
    (["--token-ids", "ids.safetensors"], "--token-ids needs --gemma-weights"),
    (["--negative-token-ids", "neg.safetensors"], "--negative-token-ids needs --token-ids"),
    (["--gemma-weights", "a.safetensors", "--token-ids", "i.safetensors", "--gemma-hidden-states", "h.safetensors"],
     "--gemma-weights is an alternative to --gemma-hidden-states and --embeddings: give one of them"),
    (["--gemma-weights"], "Missing value for '--gemma-weights'"),
])
def test_gemma_flag_validation_messages(ltx, args, msg):
    rc, _, err = run("generate", "x", "--dry-run", *args)
    assert rc != 0 and msg in err


def test_no_text_source_names_all_three(ltx):
    """Neither a hidden-states source nor Gemma weights (nor embeddings): the message names every way in. Raised before anything is
    loaded, so no GPU is needed."""
    rc, _, err = run("generate", "x", "--ltx-weights", "dit.safetensors", "--vae-weights", "vae.safetensors")
    assert rc != 0
    assert ("this build needs --ltx-weights, --vae-weights and --embeddings or --gemma-hidden-states, or --gemma-weights with --token-ids "
            "(no downloads, no tokenizer)") in err


def test_usage_lists_the_new_flags(ltx):
    rc, out, _ = run("generate", "--help")
    assert rc == 0 and "--gemma-weights file[,file...] --token-ids file [--negative-token-ids file]" in out
