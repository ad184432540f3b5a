#!/usr/bin/env python3
"""Times ONE full-width dual video + audio transformer block (ltx_dual_blocks_forward_dev; video 32 x 128 = 4096, audio 32 x 64 = 2048,
T_v = 1536 = (4, 16, 24), T_a = 126, S = 1024, B = 1) and writes profiles/dual_block_bench.txt:

  * the whole block and each of its eight phases alone (ltx_dual_forward_args.phase_mask; phases 5 and 6 each include the cross-modal
    norm launch, so their sum counts it twice - the row "5+6" runs them together);
  * the same block composed in torch bf16 (torch.nn.functional: linear, rms_norm, scaled_dot_product_attention, gelu) on the same GPU
    in the same process, alternating sample by sample with the library;
  * launch_norm_mod2 (ltx_op_norm_mod2) against the four launch_norm_mod calls it replaces (ltx_op_norm_mod_ex), at the block's shape.

Each sample is `--batch` back-to-back calls between two HIP events; the median and the minimum over `--iters` samples after `--warmup`
are reported, and the run-to-run spread of a row is (p90 - p10) / median of its samples. Run by hand:

    python tools/bench_dual_block.py [--iters 20] [--warmup 3] [--batch 10] [--out profiles/dual_block_bench.txt]
"""
import argparse
import importlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HV = HA = 32
DV, DA = HV * 128, HA * 64
FHW, T_A, S = (4, 16, 24), 126, 1024
T_V = FHW[0] * FHW[1] * FHW[2]
PHASES = ("video self-attn", "audio self-attn", "video text cross", "audio text cross", "a2v", "v2a", "video FFN", "audio FFN")


def sample(fn, batch, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch  # us per call


def stats(ts):
    ts = sorted(ts)
    med = statistics.median(ts)
    p10, p90 = ts[int(0.1 * (len(ts) - 1))], ts[int(math.ceil(0.9 * (len(ts) - 1)))]
    return med, ts[0], (p90 - p10) / med


def measure(fns, args, torch):
    """Alternates the callables sample by sample; returns one list of samples per callable."""
    out = [[] for _ in fns]
    for i in range(args.warmup + args.iters):
        for k, fn in enumerate(fns):
            t = sample(fn, args.batch, torch)
            if i >= args.warmup:
                out[k].append(t)
    return out


def torch_block(torch, w, t):
    """The eight phases in torch bf16 on resident bf16 weights (f32 streams, bf16 operands, as the library keeps them)."""
    import torch.nn.functional as F
    bf = torch.bfloat16

    def rms(x):
        return F.rms_norm(x, (x.shape[-1],), eps=1e-6)

    def rope(x, cs, heads):
        b, n, hd = x.shape
        d = hd // heads
        xh = x.view(b, n, heads, 2, d // 2)
        c, s = cs[0].view(1, n, heads, d // 2), cs[1].view(1, n, heads, d // 2)
        a, bb = xh[:, :, :, 0], xh[:, :, :, 1]
        return torch.stack([a * c - bb * s, bb * c + a * s], dim=3).reshape(b, n, hd)

    def attn(p, x, heads, context=None, qt=None, kt=None, bias=None):
        ctx = x if context is None else context
        q = F.linear(x, w[p + "to_q.weight"], w[p + "to_q.bias"]).float()
        k = F.linear(ctx, w[p + "to_k.weight"], w[p + "to_k.bias"]).float()
        v = F.linear(ctx, w[p + "to_v.weight"], w[p + "to_v.bias"])
        q, k = rms(q) * w[p + "q_norm.weight"], rms(k) * w[p + "k_norm.weight"]
        if qt is not None:
            q, k = rope(q, qt, heads), rope(k, kt if kt is not None else qt, heads)
        b, n, hd = q.shape
        qh, kh, vh = (z.to(bf).view(b, -1, heads, hd // heads).transpose(1, 2) for z in (q, k, v))
        mask = None if bias is None else bias.to(bf).view(b, 1, 1, -1)
        o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask).transpose(1, 2).reshape(b, n, hd)
        return F.linear(o, w[p + "to_out.weight"], w[p + "to_out.bias"]).float()

    def ff(p, x):
        h = F.gelu(F.linear(x, w[p + "project_in.proj.weight"], w[p + "project_in.proj.bias"]), approximate="tanh")
        return F.linear(h, w[p + "project_out.weight"], w[p + "project_out.bias"]).float()

    def run():
        xv, xa = t["xv"].clone(), t["xa"].clone()
        mv, ma = w["scale_shift_table"] + t["temb_v"], w["audio_scale_shift_table"] + t["temb_a"]
        cv, ca = w["scale_shift_table_a2v_ca_video"] + t["css_v"], w["scale_shift_table_a2v_ca_audio"] + t["css_a"]
        xv = xv + attn("attn1.", (rms(xv) * (1 + mv[:, 1:2]) + mv[:, 0:1]).to(bf), HV, qt=t["rope_v"]) * mv[:, 2:3]
        xa = xa + attn("audio_attn1.", (rms(xa) * (1 + ma[:, 1:2]) + ma[:, 0:1]).to(bf), HA, qt=t["rope_a"]) * ma[:, 2:3]
        xv = xv + attn("attn2.", rms(xv).to(bf), HV, context=t["ctx_v"], bias=t["bias_v"])
        xa = xa + attn("audio_attn2.", rms(xa).to(bf), HA, context=t["ctx_a"], bias=t["bias_a"])
        nv, na = rms(xv), rms(xa)
        xv = xv + attn("audio_to_video_attn.", (nv * (1 + cv[:, 0:1]) + cv[:, 1:2]).to(bf), HA, context=(na * (1 + ca[:, 0:1]) + ca[:, 1:2]).to(bf),
                       qt=t["rope_cv"], kt=t["rope_ca"]) * cv[:, 4:5]
        xa = xa + attn("video_to_audio_attn.", (na * (1 + ca[:, 2:3]) + ca[:, 3:4]).to(bf), HA, context=(nv * (1 + cv[:, 2:3]) + cv[:, 3:4]).to(bf),
                       qt=t["rope_ca"], kt=t["rope_cv"]) * ca[:, 4:5]
        xv = xv + ff("ff.", (rms(xv) * (1 + mv[:, 4:5]) + mv[:, 3:4]).to(bf)) * mv[:, 5:6]
        xa = xa + ff("audio_ff.", (rms(xa) * (1 + ma[:, 4:5]) + ma[:, 3:4]).to(bf)) * ma[:, 5:6]
        return xv, xa

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    ctx = ltx.Context(0)
    ctx.dual_blocks_init_synthetic(ltx.default_dual_block_config(num_layers=1), seed=9)
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    t = {"xv": rn(1, T_V, DV), "xa": rn(1, T_A, DA), "ctx_v": (2 * rn(1, S, DV)).to(torch.bfloat16), "ctx_a": (2 * rn(1, S, DA)).to(torch.bfloat16),
         "temb_v": 0.3 * rn(1, 6, DV), "temb_a": 0.3 * rn(1, 6, DA), "css_v": 0.3 * rn(1, 5, DV), "css_a": 0.3 * rn(1, 5, DA)}
    for k, r in (("temb_v", 2), ("temb_v", 5), ("temb_a", 2), ("temb_a", 5), ("css_v", 4), ("css_a", 4)):
        t[k][:, r] += 1.0
    for n in ("v", "a"):
        t["bias_" + n] = torch.zeros((1, S), device="cuda")
        t["bias_" + n][:, S - S // 3:] = -10000.0
    xv, xa = t["xv"].clone(), t["xa"].clone()

    def ours(mask=0):
        # in place on scratch copies of the streams: values drift over repeated calls but stay finite (gates of order 1, one block);
        # the kernels' time does not depend on the values
        return lambda: ctx.dual_blocks_forward_dev(xv, xa, t["ctx_v"], t["ctx_a"], t["temb_v"], t["temb_a"], t["css_v"], t["css_a"], *FHW,
                                                   key_bias_video=t["bias_v"], key_bias_audio=t["bias_a"], phase_mask=mask)

    def reset():
        xv.copy_(t["xv"])
        xa.copy_(t["xa"])

    # torch side: the same weights (exported once), bf16 matrices, f32 biases / tables
    import numpy as np
    names = {}
    for a in ("attn1", "attn2", "audio_attn1", "audio_attn2", "audio_to_video_attn", "video_to_audio_attn"):
        for n in ("to_q", "to_k", "to_v", "to_out"):
            names[f"{a}.{n}.weight"] = names[f"{a}.{n}.bias"] = None
        names[f"{a}.q_norm.weight"] = names[f"{a}.k_norm.weight"] = None
    for f in ("ff", "audio_ff"):
        for n in ("project_in.proj", "project_out"):
            names[f"{f}.{n}.weight"] = names[f"{f}.{n}.bias"] = None
    for n in ("scale_shift_table", "audio_scale_shift_table", "scale_shift_table_a2v_ca_video", "scale_shift_table_a2v_ca_audio"):
        names[n] = None
    w = {}
    for k in names:
        v = torch.from_numpy(ctx.dual_blocks_export_param("transformer_blocks.0." + k)).cuda()
        if k.endswith(".weight") and "_norm." not in k:  # [out][in]: `out` is the length of the companion bias
            b = ctx.dual_blocks_export_param("transformer_blocks.0." + k[:-len("weight")] + "bias").size
            w[k] = v.view(b, -1).to(torch.bfloat16)
        elif k.endswith(".bias"):
            w[k] = v.to(torch.bfloat16)
        elif "scale_shift_table" in k:
            w[k] = v.view(1, 6 if k in ("scale_shift_table", "audio_scale_shift_table") else 5, -1)
        else:
            w[k] = v
    tab = lambda cs: tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in cs)  # noqa: E731
    cfg = ltx.default_transformer_config()
    t["rope_v"] = tab(ltx.rope_tables(cfg, *FHW))
    t["rope_a"] = tab(ltx.rope_tables_positions(ltx.audio_positions(T_A), DA))
    t["rope_ca"] = t["rope_a"]
    t["rope_cv"] = tab(ltx.rope_tables_positions(ltx.video_temporal_positions(*FHW), DA))
    tb = torch_block(torch, w, t)

    lines = [f"dual video + audio block, full width: Dv {DV} (32 x 128), Da {DA} (32 x 64), T_v {T_V} {FHW}, T_a {T_A}, S {S}, B 1, one block; us per call, "
             f"median / min of {args.iters} samples of {args.batch} calls after {args.warmup} warm-up samples; spread = (p90 - p10) / median; "
             f"torch {torch.__version__}",
             f"{'row':<34}{'median us':>12}{'min us':>12}{'spread':>9}"]
    row = lambda name, ts: lines.append("{:<34}{:>12.1f}{:>12.1f}{:>8.1f}%".format(name, stats(ts)[0], stats(ts)[1], 100 * stats(ts)[2]))  # noqa: E731

    # parity of the two compositions before anything is timed
    reset()
    ours()()
    tv, ta = tb()
    torch.cuda.synchronize()
    dv = ((xv - tv).norm() / tv.norm()).item()
    da = ((xa - ta).norm() / ta.norm()).item()
    reset()
    whole, torch_t = measure([ours(), tb], args, torch)
    row("whole block (library)", whole)
    row("whole block (torch bf16)", torch_t)
    lines.append(f"library / torch = {stats(whole)[0] / stats(torch_t)[0]:.3f}; the two results differ by rel-L2 {dv:.2e} (video) / {da:.2e} (audio) after one block")
    reset()
    per = measure([ours(1 << p) for p in range(8)] + [ours(0x30)], args, torch)
    for name, ts in zip(PHASES + ("5+6 together",), per):
        row("phase " + name, ts)
    lines.append(f"sum of the eight phase medians {sum(stats(x)[0] for x in per[:8]):.1f} us (counts the cross-modal norm launch twice and the four "
                 "modulation-table launches eight times)")

    # the cross-modal norms: one launch_norm_mod2 against the four launch_norm_mod passes it replaces
    def job(D, rows):
        return {"x": rn(rows, D), "rows": rows, "D": D, "scale0": 0.3 * rn(D), "shift0": 0.3 * rn(D), "scale1": 0.3 * rn(D), "shift1": 0.3 * rn(D),
                "out0": torch.empty((rows, D), device="cuda", dtype=torch.bfloat16), "out1": torch.empty((rows, D), device="cuda", dtype=torch.bfloat16)}
    jv, ja = job(DV, T_V), job(DA, T_A)
    rv = [torch.empty_like(jv["out0"]), torch.empty_like(jv["out1"])]
    ra = [torch.empty_like(ja["out0"]), torch.empty_like(ja["out1"])]

    def four():
        for j, r in ((jv, rv), (ja, ra)):
            ctx.op_norm_mod_ex(j["x"], j["scale0"], j["shift0"], r[0], j["rows"], j["D"])
            ctx.op_norm_mod_ex(j["x"], j["scale1"], j["shift1"], r[1], j["rows"], j["D"])

    one = lambda: ctx.op_norm_mod2(jv, ja)  # noqa: E731
    one()
    four()
    torch.cuda.synchronize()
    equal = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in ((jv["out0"], rv[0]), (jv["out1"], rv[1]), (ja["out0"], ra[0]), (ja["out1"], ra[1])))
    nargs = argparse.Namespace(iters=args.iters, warmup=args.warmup, batch=max(args.batch, 50))
    t1, t4 = measure([one, four], nargs, torch)
    row("launch_norm_mod2 (1 launch)", t1)
    row("4 x launch_norm_mod", t4)
    m1, m4 = stats(t1), stats(t4)
    verdict = "not slower: selected" if m1[0] <= m4[0] * (1 + max(m1[2], m4[2])) else "SLOWER beyond the spread: the block must call the four passes"
    lines.append(f"norm_mod2 / four passes = {m1[0] / m4[0]:.3f} (samples of {nargs.batch} calls); outputs bit-equal: {equal}; {verdict}")
    lines.append("Each call is issued from Python through ctypes: rows of a few microseconds sit at the host's issue rate, not at the kernel's time.")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.dual_blocks_unload()
    ctx.close()


if __name__ == "__main__":
    main()
