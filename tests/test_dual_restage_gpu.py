"""ltx_op_dual_restage alone (dual_restage_kernel, csrc/elementwise.hip): the bridge between the two stages of the two-stage video + audio
path - AdaIN at factor 1, the re-noise of both streams, frame 0 of an image-to-video run, token layout and the bf16 cast in one launch.

Exact: against the numpy float32 replay of tests/helpers/dual_two_stage_ref.py fed the hook's own stats_out, the f32 latents and the bf16
tokens are bit-equal - video only, audio only, both; without an image latent, with one, with its re-noise slice; T in {32, 96, 100} (100
is no multiple of the 32-token tile) at C = 128, and one full-width case T = 1536. The statistics themselves: the video output before
re-noise (s = 0) against Context.adain_filter_latent within the project's AdaIN bound, max abs <= 1e-4 (tests/test_two_stage_gpu.py).
Refusals write nothing; a null job is allowed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_two_stage_ref as ts  # noqa: E402

pytestmark = pytest.mark.gpu
C = 128
T_A = 26
S_NOISE = 0.909375
COND_SCALE = 0.5


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def bits(tok):
    return tok.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def data():
    """Inputs for every T, once; shared and left unchanged. The upscaled latent has its own mean and spread per channel."""
    rng = np.random.default_rng(11)
    d = {}
    for T in (32, 96, 100, 1536):
        scale = (0.5 + 1.5 * rng.random((C, 1))).astype(np.float32)
        shift = (0.6 * rng.standard_normal((C, 1))).astype(np.float32)
        HW = T // 4 if T == 1536 else T // 2
        d[T] = {"x": (rng.standard_normal((C, T)).astype(np.float32) * scale + shift).astype(np.float32),
                "ref": rng.standard_normal((C, max(T // 4, 4))).astype(np.float32), "noise": rng.standard_normal((C, T)).astype(np.float32),
                "cond": rng.standard_normal((C, HW)).astype(np.float32), "cond_noise": rng.standard_normal((C, HW)).astype(np.float32)}
    d["audio"] = rng.standard_normal((T_A, C)).astype(np.float32)
    d["audio_noise"] = rng.standard_normal((T_A, C)).astype(np.float32)
    return d


def run(ctx, data, T=None, audio=False, cond_mode="none", s=S_NOISE, noise=True):
    """One call on fresh device tensors; returns what it wrote and what the replay makes of the same inputs and of the hook's statistics."""
    got, want = {}, {}
    vj = aj = None
    if T is not None:
        d = data[T]
        lat, tok = torch.full((T, C), 7.0, device="cuda"), torch.zeros((T, C), device="cuda", dtype=torch.bfloat16)
        stats = torch.zeros(4 * C, device="cuda")
        vj = dict(x=dev(d["x"]), latent=lat, tokens=tok, ref=dev(d["ref"]), stats_out=stats, noise=dev(d["noise"]) if noise else None, noise_scale=s)
        kw = {}
        if cond_mode != "none":
            vj["cond"] = dev(d["cond"])
            kw["cond"] = d["cond"]
        if cond_mode == "cond_noise":
            s2 = np.float32(np.float32(s) * np.float32(s))
            vj.update(cond_noise=dev(d["cond_noise"]), cond_scale=COND_SCALE, cond_sigma2=float(s2))
            kw.update(cond_noise=d["cond_noise"], cond_scale=COND_SCALE, cond_sigma2=s2)
    if audio:
        alat, atok = dev(data["audio"]), torch.zeros((T_A, C), device="cuda", dtype=torch.bfloat16)
        aj = dict(latent=alat, tokens=atok, noise=dev(data["audio_noise"]) if noise else None, noise_scale=s)
    ctx.op_dual_restage(vj, aj)
    torch.cuda.synchronize()
    if T is not None:
        st = stats.cpu().numpy().reshape(2, C, 2)
        got["video"], got["video_tok"], got["stats"] = lat.cpu().numpy(), bits(tok), st
        want["video"], want["video_tok"] = ts.restage_video(d["x"], st[0], st[1], d["noise"] if noise else None, s, **kw)
    if audio:
        got["audio"], got["audio_tok"] = alat.cpu().numpy(), bits(atok)
        want["audio"], want["audio_tok"] = ts.restage_audio(data["audio"], data["audio_noise"] if noise else None, s)
    return got, want


def check(got, want):
    for k in want:
        if k.endswith("_tok"):
            assert np.array_equal(got[k], want[k]), k
        else:
            assert np.isfinite(got[k]).all() and same_bits(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))


@pytest.mark.parametrize("cond_mode", ["none", "cond", "cond_noise"])
@pytest.mark.parametrize("T", [32, 96, 100])
def test_both_jobs_equal_the_float32_replay_bit_for_bit(gpu_ctx, data, T, cond_mode):
    got, want = run(gpu_ctx, data, T, audio=True, cond_mode=cond_mode)
    check(got, want)
    HW = data[T]["cond"].shape[1]
    if cond_mode == "cond":  # no AdaIN or re-noise result survives for frame-0 tokens
        assert same_bits(got["video"][:HW], data[T]["cond"].T)
    plain = ts.restage_video(data[T]["x"], got["stats"][0], got["stats"][1], data[T]["noise"], S_NOISE)[0]
    assert same_bits(got["video"][HW:], plain[HW:])
    assert (cond_mode == "none") == same_bits(got["video"][:HW], plain[:HW])


@pytest.mark.parametrize("which", ["video", "audio"])
def test_one_job_alone(gpu_ctx, data, which):
    got, want = run(gpu_ctx, data, 100 if which == "video" else None, audio=which == "audio", cond_mode="cond_noise")
    assert set(want) == {which, which + "_tok"}
    check(got, want)


def test_full_width(gpu_ctx, data):
    """T = 1536 (stage 2 of the benchmark shape, (4, 16, 24)): 192 video workgroups and the audio job, frame 0 re-noised."""
    got, want = run(gpu_ctx, data, 1536, audio=True, cond_mode="cond_noise")
    check(got, want)


def test_without_a_noise_scale_the_blend_is_skipped(gpu_ctx, data):
    """renoise = 0 with no noise is a valid call: AdaIN and the cast alone; the audio latent is left as it is."""
    got, want = run(gpu_ctx, data, 96, audio=True, noise=False)
    check(got, want)
    assert same_bits(got["audio"], data["audio"])


def test_the_statistics_are_those_of_adain_filter_latent(gpu_ctx, data):
    """s = 0 leaves the AdaIN output: held against ltx_adain_filter_latent (two launch_mean_var and launch_adain) within max abs 1e-4."""
    T = 96
    got, want = run(gpu_ctx, data, T, s=0.0)
    check(got, want)
    x5, r5 = data[T]["x"].reshape(1, C, 2, 6, 8), data[T]["ref"].reshape(1, C, 2, 3, 4)
    lib = gpu_ctx.adain_filter_latent(x5, r5, 1.0).reshape(C, T)
    err = float(np.abs(got["video"].T - lib).max())
    print(f"restage at s = 0 against ltx_adain_filter_latent: max abs {err:.3e}")
    assert err <= 1e-4
    # and the statistics are what numpy takes from the same arrays
    assert np.abs(got["stats"][0] - ts.mean_var(data[T]["x"])).max() <= 1e-4 and np.abs(got["stats"][1] - ts.mean_var(data[T]["ref"])).max() <= 1e-4


def test_given_statistics_are_used_and_returned(gpu_ctx, data):
    T = 100
    d = data[T]
    st, sr = ts.mean_var(d["x"]), ts.mean_var(d["ref"])
    lat, tok = torch.empty((T, C), device="cuda"), torch.empty((T, C), device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(4 * C, device="cuda")
    gpu_ctx.op_dual_restage(dict(x=dev(d["x"]), latent=lat, tokens=tok, stats=dev(st), stats_ref=dev(sr), stats_out=out, noise=dev(d["noise"]),
                                 noise_scale=S_NOISE))
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy().reshape(2, C, 2), np.stack([st, sr]))
    want, wtok = ts.restage_video(d["x"], st, sr, d["noise"], S_NOISE)
    assert same_bits(lat.cpu().numpy(), want) and np.array_equal(bits(tok), wtok)


def test_refusals_write_nothing_and_null_jobs_are_allowed(gpu_ctx, ltx, data):
    gpu_ctx.op_dual_restage(None, None)  # nothing to do
    T = 96
    d = data[T]
    lat, tok = torch.full((T, C), 7.0, device="cuda"), torch.full((T, C), 3.0, device="cuda", dtype=torch.bfloat16)
    stats = torch.full((4 * C,), 5.0, device="cuda")
    alat, atok = dev(data["audio"]), torch.full((T_A, C), 3.0, device="cuda", dtype=torch.bfloat16)
    good = dict(x=dev(d["x"]), latent=lat, tokens=tok, ref=dev(d["ref"]), stats_out=stats, noise=dev(d["noise"]), noise_scale=S_NOISE)
    agood = dict(latent=alat, tokens=atok, noise=dev(data["audio_noise"]), noise_scale=S_NOISE)
    bad = [(dict(good, C=48, T=T), agood), (dict(good, latent=None, C=C, T=T), agood), (dict(good, tokens=None), agood),
           (dict(good, cond=dev(d["cond"]), HW=T + 1), agood), (dict(good, cond_noise=dev(d["cond_noise"])), agood),
           (dict(good, noise=None, renoise=1), agood), (dict(good, renoise=0), agood), (dict(good, ref=None), agood),
           (dict(good, stats=stats), agood), (good, dict(agood, noise=None, renoise=1)), (good, dict(agood, C=100, T=T_A)),
           (good, dict(agood, x=dev(d["x"])))]
    for vj, aj in bad:
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.op_dual_restage(vj, aj)
        assert e.value.case == "invalidConfiguration"
    torch.cuda.synchronize()
    assert bool((lat == 7.0).all()) and bool((tok == 3.0).all()) and bool((stats == 5.0).all()) and bool((atok == 3.0).all())
    assert torch.equal(alat, dev(data["audio"])), "a refused call wrote"
    gpu_ctx.op_dual_restage(good, agood)  # and the same jobs, unspoiled, pass
    torch.cuda.synchronize()
    assert not bool((lat == 7.0).any())
