"""Fixtures of the bit-exact LoRA fusion / requantisation / encoder tests (test_lora_exact_gpu.py, test_quant_adversarial_gpu.py,
test_text_cache_refresh_gpu.py) and of the CPU test that keeps their preconditions (test_lora_quant_fixtures_host.py).

LoRA factors are small integers times a power of two, drawn so that sum_r |up[o, r]| * |down[r, i]| <= 256 for every output element:
every partial sum of up @ down is then an integer below 2^8 (times a power of two), exact in bf16 and f32 alike, so the delta does not
depend on the accumulation order, the rank padding, a K split or bf16 partials. What is left of the merge is three single f32
operations with one bf16 rounding each, which numpy float32 (oracle.lora_fuse) reproduces bit for bit."""
import math
from collections import namedtuple

import numpy as np

HEADS, LAYERS, CAPTION = 2, 2, 128          # the small model of test_lora_quant_gpu._setup: D = 256, FFN 1024
FRAMES, HEIGHT, WIDTH, TEXT = 2, 3, 4, 19   # T = 24 tokens, S = 19 text tokens
BOUND = 256

# rank, alpha (None: no .alpha tensor), fuse scale, key spelling ("down": lora_down / lora_up, "A": lora_A / lora_B), ".weight" suffix
Recipe = namedtuple("Recipe", "rank alpha scale spelling suffix seed")
RECIPES = {
    "r1": Recipe(1, None, 1.0, "down", True, 11),
    "r16-alpha": Recipe(16, 8.0, 0.8, "A", True, 12),
    "r64": Recipe(64, None, 0.8, "down", False, 13),         # no alpha: eff is the fuse scale alone, and bf16(delta * 0.8) rounds
    "r65-alpha": Recipe(65, 8.0, 0.8, "A", False, 14),      # eff = 0.8 * (8 / 65): neither factor a power of two
    "r160-alpha": Recipe(160, 16.0, 1.0, "down", True, 15),  # padded to 192; sparser factors keep the bound
}


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32).ravel(), np.ascontiguousarray(b, dtype=np.float32).ravel()
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def reachable_linears(ocfg):
    """[(LoRA base key as a file spells it, module weight key, out, in)]: every Linear of the DiT that map_lora_key can reach."""
    D = ocfg.dim
    lin = [("adaln_single.emb.timestep_embedder.linear_1", "adaln_single.emb.linear_1", D, 256),
           ("adaln_single.emb.timestep_embedder.linear_2", "adaln_single.emb.linear_2", D, D),
           ("adaln_single.linear", "adaln_single.linear", 6 * D, D),
           ("caption_projection.linear_1", "caption_projection.linear_1", D, ocfg.caption_channels),
           ("caption_projection.linear_2", "caption_projection.linear_2", D, D),
           ("proj_out", "proj_out", ocfg.out_channels, D)]
    for i in range(ocfg.num_layers):
        p = f"transformer_blocks.{i}."
        for a in ("attn1", "attn2"):
            for l in ("to_q", "to_k", "to_v"):
                lin.append((p + f"{a}.{l}", p + f"{a}.{l}", D, D))
            lin.append((p + f"{a}.to_out.0", p + f"{a}.to_out", D, D))
        lin.append((p + "ff.net.0.proj", p + "ff.project_in.proj", 4 * D, D))
        lin.append((p + "ff.net.2", p + "ff.project_out", D, 4 * D))
    return [("diffusion_model." + b, m + ".weight", o, i) for b, m, o, i in lin]


def exact_factors(rng, out, inn, rank):
    """Integer factors: up in {-1, 0, 1}, down in {-2 .. 2}. Below rank 8 without zeros (the product would leave too many elements
    alone), above rank 100 with half of `up` zeroed (dense, the bound 2 * rank would pass 256)."""
    if rank < 8:
        up = rng.choice(np.array([-1, 1]), (out, rank))
        down = rng.choice(np.array([-2, -1, 1, 2]), (rank, inn))
    else:
        up = rng.integers(-1, 2, (out, rank))
        down = rng.integers(-2, 3, (rank, inn))
        if rank > 100:
            up = up * (rng.random((out, rank)) < 0.5)
    return up.astype(np.int64), down.astype(np.int64)


def partial_sum_bound(up_int, down_int):
    """max over output elements of sum_r |up[o, r]| * |down[r, i]|: no partial sum of up @ down, in any order, exceeds it."""
    return int((np.abs(up_int) @ np.abs(down_int)).max())


def make_exact_lora(recipe, layers, extras=True):
    """-> (file dict, meta). `layers`: entries of reachable_linears to name. meta[module key] = (up_int, down_int, shift_up, shift_down):
    the file holds up_int * 2^-shift_up and down_int * 2^-shift_down, exact in f32, bf16 and f16. The shifts bring the scaled delta to
    about 0.6 / sqrt(in), the size of the weights, so that the merge rounds and neither vanishes nor swamps.
    extras: also the keys a loader must pass over - `proj_in` (the file's name of patchify_proj, which map_lora_key does not
    translate), a layer without its `up` half and a layer whose .alpha has two elements (ignored: the fuse scale alone applies)."""
    rng = np.random.default_rng(recipe.seed)
    dn, un = ("lora_down", "lora_up") if recipe.spelling == "down" else ("lora_A", "lora_B")
    sfx = ".weight" if recipe.suffix else ""
    eff = np.float32(recipe.scale)
    if recipe.alpha is not None:
        eff = np.float32(recipe.scale) * (np.float32(recipe.alpha) / np.float32(recipe.rank))
    lora, meta = {}, {}
    for base, mk, out, inn in layers:
        up, down = exact_factors(rng, out, inn, recipe.rank)
        shift = int(round(math.log2(float((up @ down).std()) * float(eff) / (0.6 / math.sqrt(inn)))))
        su, sd = shift // 2, shift - shift // 2
        lora[f"{base}.{dn}{sfx}"] = (down * 2.0 ** -sd).astype(np.float32)
        lora[f"{base}.{un}{sfx}"] = (up * 2.0 ** -su).astype(np.float32)
        if recipe.alpha is not None:
            lora[base + ".alpha"] = np.array(recipe.alpha, np.float32)
        meta[mk] = (up, down, su, sd)
    if extras:
        r = recipe.rank
        lora[f"diffusion_model.proj_in.{dn}{sfx}"] = np.ones((r, 128), np.float32)
        lora[f"diffusion_model.proj_in.{un}{sfx}"] = np.ones((layers[0][2], r), np.float32)
    return lora, meta


def drop_up_half(lora, base):
    """The layer keeps its down / A matrix only: parseLoRALayers finds no pair and passes over it."""
    for k in [k for k in lora if k.startswith(base + ".") and (".lora_up" in k or ".lora_B" in k)]:
        del lora[k]


def oracle_fuse(oracle, w, lora, scale):
    """oracle.lora_fuse, with the loader's reading of .alpha: a tensor of more than one element is not an alpha."""
    return oracle.lora_fuse(w, {k: v for k, v in lora.items() if not (k.endswith(".alpha") and np.size(v) != 1)}, scale)


def fused_module_keys(oracle, w, lora):
    """Module keys a file changes: both halves present and the mapped key exists in the model."""
    keys = set()
    for k in lora:
        for dn, un in (("lora_down", "lora_up"), ("lora_A", "lora_B")):
            if dn in k and k.replace(dn, un) in lora:
                mk = oracle.map_lora_key(k.replace(f".{dn}.weight", "").replace(f".{dn}", ""))
                if mk in w:
                    keys.add(mk)
    return keys


def requant_reference(oracle, w, lora, scale, bits, keys):
    """dequant -> merge -> requant of the fused keys, all numpy float32: wq = bf16(fake_quant(W)) is what quant_decode_kernel writes,
    merged = bf16(wq + d) what lora_add_kernel leaves, want = bf16(fake_quant(merged)) what the slot exports after the re-encode."""
    wq = {k: oracle.bf16_round(oracle.fake_quant(w[k], bits)) for k in keys}
    merged, _ = oracle_fuse(oracle, wq, lora, scale)
    return wq, {k: oracle.bf16_round(oracle.fake_quant(merged[k], bits)) for k in keys}


def changed_group_share(a, b):
    return float((a.reshape(-1, 64) != b.reshape(-1, 64)).any(1).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted 64-element groups for the encoder: each decides one data-dependent branch of quant_encode_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def crafted_groups(oracle, large=1e30):
    rng = np.random.default_rng(3)
    r = oracle.bf16_round
    g = rng.standard_normal(64).astype(np.float32)
    groups = {}
    groups["zero"] = np.zeros(64, np.float32)
    groups["const_pos"] = np.full(64, 0.07, np.float32)
    groups["const_neg"] = np.full(64, -0.07, np.float32)
    groups["pos_outlier"] = np.zeros(64, np.float32)
    groups["pos_outlier"][17] = 0.5
    groups["neg_outlier"] = np.zeros(64, np.float32)
    groups["neg_outlier"][40] = -0.5
    sym = np.clip(g * 0.04, -0.09, 0.09)
    sym[3], sym[9] = 0.1, -0.1
    groups["abs_min_eq_abs_max"] = sym
    groups["all_pos"] = np.abs(g) * 0.05 + 0.01
    groups["all_neg"] = -(np.abs(g) * 0.05 + 0.01)
    groups["under_floor"] = np.where(np.arange(64) % 2 == 0, 0.0, 2.0 ** -30).astype(np.float32)   # range / 255 < 1e-7
    groups["tiny_normal"] = r(g) * np.float32(2.0 ** -100)
    groups["large"] = g * np.float32(large)
    groups["two_adjacent"] = np.where(rng.random(64) < 0.5, 1.0, 1.0078125).astype(np.float32)
    groups["int_ramp"] = np.arange(-32, 32).astype(np.float32)
    # 8 bits: w_min = 0, w_max = 255 / 256, so scale = -2^-8 and bias = w_max exactly; (w - bias) / scale = 254.5 - k on every other value
    half = np.array([0.0, 255.0 / 256.0] + [(2 * k + 1) / 512.0 for k in range(1, 125, 2)], np.float32)
    groups["half_steps"] = half[rng.permutation(64)]
    out = {}
    for k, v in groups.items():
        v = r(np.asarray(v, np.float32))
        assert v.shape == (64,)
        out[k] = v
    assert np.array_equal(out["half_steps"], groups["half_steps"]) and np.array_equal(out["under_floor"], groups["under_floor"])
    return out


ADVERSARIAL_KEYS = ("transformer_blocks.0.ff.project_in.proj.weight", "transformer_blocks.1.attn1.to_q.weight",
                    "transformer_blocks.1.attn1.to_k.weight")


def plant_groups(w, groups):
    """Copy of the weight dict with the crafted groups written over whole 64-element groups of ADVERSARIAL_KEYS: at the start and at
    the end of each matrix (first row, last row; for to_q | to_k that is either side of the view boundary inside the fused matrix and
    its last row) and, in the FFN matrix, scattered through the middle. -> (weights, {key: group indices written})."""
    out = dict(w)
    vals = list(groups.values())
    where = {}
    for key in ADVERSARIAL_KEYS:
        m = out[key].astype(np.float32).copy()
        flat = m.reshape(-1, 64)
        n = flat.shape[0]
        idx = list(range(len(vals))) + list(range(n - len(vals), n))
        if "ff." in key:
            idx += [(293 * (j + 1)) % (n - 2 * len(vals)) + len(vals) for j in range(len(vals))]
        assert len(set(idx)) == len(idx)
        for j, gi in enumerate(idx):
            flat[gi] = vals[j % len(vals)]
        out[key] = m
        where[key] = idx
    return out, where
