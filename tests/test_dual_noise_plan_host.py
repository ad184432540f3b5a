"""The draw plan of a video + audio generation (csrc/dual_generate.cpp, ltx_dual_noise_plan) and the key split the host and the device
generator share (ltx_mlx_draw_key). Pure host code: the reference draws every tensor of a run from one seeded key sequence in a fixed
order (LTXPipeline.swift:1225-1236, :1291, :1572-1581, :1629, :1730-1734, :1766), and the plan is that order, written out here by hand."""
import ctypes

import numpy as np
import pytest

C, F, H, W, T_A, S = 128, 2, 3, 4, 26, 70
V1, A1, K1, V2, A2, K2 = range(6)  # LTX_NOISE_VIDEO1 .. LTX_NOISE_COND2
SIGMAS1 = [1.0, 0.725, 0.25, 0.0]
SIGMAS2 = [0.909375, 0.725, 0.421875, 0.0]
FRAME, VIDEO, AUDIO = C * H * W, C * F * H * W, 128 * T_A


def make(ltx, two_stage=False, i2v=False, scale=0.0, sigmas1=SIGMAS1, sigmas2=None, **kw):
    cond = np.zeros(1, np.float32)  # the plan reads the image latents as flags
    base = dict(seed=7, F=F, H=H, W=W, T_a=T_A, S=S, sigmas1=sigmas1, two_stage=two_stage, sigmas2=sigmas2, channels=C,
                cond_latent1=cond if i2v else None, cond_latent2=cond if i2v and two_stage else None, image_cond_noise_scale=scale)
    base.update(kw)
    return ltx.dual_generate_args(**base)


def rows(plan):
    return [(d["draw_index"], d["role"], d["step"], d["numel"]) for d in plan]


def test_draw_key_is_the_oracles_key_split(ltx, oracle):
    for seed in (0, 42, 2**40 + 5):
        g = (np.uint32((seed >> 32) & 0xFFFFFFFF), np.uint32(seed & 0xFFFFFFFF))
        subs = []
        for _ in range(8):  # oracle.mlx_random_normal's split: row 0 stays global, row 1 is the draw's key
            w = oracle.mlx_random_bits(g, 4)
            g = (w[0], w[1])
            subs.append((int(w[2]), int(w[3])))
        for draw in (0, 1, 7):
            assert tuple(int(v) for v in ltx.mlx_draw_key(seed, draw)) == subs[draw], (seed, draw)
    with pytest.raises(ltx.LTXError):
        ltx.mlx_draw_key(1, -1)


def test_the_host_generator_still_draws_from_that_key(ltx, oracle):
    """mlx_random_normal now takes its key from the shared split: same values as the oracle's restatement, all draws."""
    for seed, n, draw in [(42, 257, 0), (2**40 + 5, 64, 3)]:
        np.testing.assert_allclose(ltx.mlx_random_normal(seed, (n,), draw), oracle.mlx_random_normal(seed, (n,), draw), rtol=2e-6, atol=1e-7)


CASES = {
    "t2v one-stage": (dict(), [(0, V1, 0, VIDEO), (1, A1, 0, AUDIO)]),
    "i2v+renoise one-stage": (dict(i2v=True, scale=0.5),
                              [(0, V1, 0, VIDEO), (1, A1, 0, AUDIO), (2, K1, 0, FRAME), (3, K1, 1, FRAME), (4, K1, 2, FRAME)]),
    "t2v two-stage": (dict(two_stage=True), [(0, V1, 0, VIDEO), (1, A1, 0, AUDIO), (2, V2, 0, 4 * VIDEO), (3, A2, 0, AUDIO)]),
    "i2v+renoise two-stage": (dict(two_stage=True, i2v=True, scale=0.5, sigmas2=SIGMAS2),
                              [(0, V1, 0, VIDEO), (1, A1, 0, AUDIO), (2, K1, 0, FRAME), (3, K1, 1, FRAME), (4, K1, 2, FRAME),
                               (5, V2, 0, 4 * VIDEO), (6, A2, 0, AUDIO), (7, K2, 0, 4 * FRAME), (8, K2, 1, 4 * FRAME), (9, K2, 2, 4 * FRAME)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_the_references_order_of_drawing(ltx, name):
    kw, want = CASES[name]
    plan, total = ltx.dual_noise_plan(make(ltx, **kw))
    assert rows(plan) == want
    for d in plan:  # the first two draws carry the reference's separate `noise * sigmas[0]`, the others are used as drawn
        assert d["scale"] == (np.float32(SIGMAS1[0]) if d["role"] in (V1, A1) else 1.0)
    # what the loop takes in place has no slot: the audio noise always, the video noise unless stage 1 has a buffer of its own
    in_place = {A1} if kw.get("two_stage") else {V1, A1}
    assert {d["role"] for d in plan if d["offset"] < 0} == in_place
    slots = sorted((d["offset"], d["numel"], d["role"], d["step"]) for d in plan if d["offset"] >= 0)
    end = 0
    for off, n, role, step in slots:
        assert off >= end, (name, off, end)  # no overlap
        if role in (K1, K2) and step > 0:
            assert off == end  # the slices of a stage are one array to the loop
        else:
            assert off % 64 == 0
        end = off + n
    assert total >= end and total % 64 == 0 and total - end < 64


def test_the_headline_i2v_two_stage_run_makes_15_draws(ltx):
    """8 stage-1 steps and the 3 distilled stage-2 steps: 2 + 8 + 2 + 3."""
    a = make(ltx, two_stage=True, i2v=True, scale=0.3, sigmas1=np.linspace(1.0, 0.0, 9))
    plan, _ = ltx.dual_noise_plan(a)
    assert len(plan) == 15 and [d["draw_index"] for d in plan] == list(range(15))
    assert [d["role"] for d in plan] == [V1, A1] + [K1] * 8 + [V2, A2] + [K2] * 3


def test_an_image_latent_without_a_noise_scale_draws_no_slices(ltx):
    for two_stage in (False, True):
        plan, _ = ltx.dual_noise_plan(make(ltx, two_stage=two_stage, i2v=True, scale=0.0))
        assert all(d["role"] not in (K1, K2) for d in plan) and len(plan) == (4 if two_stage else 2)
    plan, _ = ltx.dual_noise_plan(make(ltx, i2v=False, scale=0.5))  # a scale without an image latent: nothing to re-noise
    assert len(plan) == 2


def test_slots_are_aligned_when_a_frame_is_no_multiple_of_64(ltx):
    a = make(ltx, two_stage=True, i2v=True, scale=0.5, channels=32, H=3, W=5, T_a=3)  # frame = 480, audio = 384
    plan, total = ltx.dual_noise_plan(a)
    offs = {(d["role"], d["step"]): d["offset"] for d in plan}
    assert offs[(V1, 0)] == 0 and offs[(K1, 0)] == 960 and offs[(K1, 1)] == 960 + 480 and offs[(K1, 2)] == 960 + 960
    assert offs[(V2, 0)] == 2432  # 960 + 3 * 480 = 2400, to the next multiple of 64
    assert offs[(A2, 0)] == 2432 + 3840 and offs[(K2, 0)] == 2432 + 3840 + 384 and total == 6656 + 3 * 1920  # = 194 * 64


def test_a_short_array_gets_the_count_and_is_not_written(ltx):
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    a = make(ltx, two_stage=True)
    arr = (lib_mod.NoiseDraw * 4)()
    for d in arr:
        d.role = -7
    total = ctypes.c_long(-1)
    assert ltx.lib.ltx_dual_noise_plan(ctypes.byref(a), arr, 3, ctypes.byref(total)) == 4
    assert all(d.role == -7 for d in arr) and total.value > 0
    assert ltx.lib.ltx_dual_noise_plan(ctypes.byref(a), arr, 4, None) == 4 and [d.role for d in arr] == [V1, A1, V2, A2]


def test_refusals(ltx):
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    plan = ltx.lib.ltx_dual_noise_plan
    bad = -2  # -LTX_ERR_INVALID_CONFIGURATION
    assert plan(None, None, 0, None) == bad
    for kw in (dict(F=0), dict(H=0), dict(W=-1), dict(T_a=0), dict(channels=0), dict(sigmas1=[1.0]), dict(sigmas1=None),
               dict(two_stage=True, sigmas2=[0.9]), dict(struct_size=ctypes.sizeof(lib_mod.DualGenerateArgs) - 24), dict(struct_size=0),
               dict(F=64, H=1024, W=1024)):  # 2^33 values in one draw: the counters are 32 bit
        assert plan(ctypes.byref(make(ltx, **kw)), None, 0, None) == bad, kw
    one = np.zeros(1, np.float32)
    assert plan(ctypes.byref(make(ltx, two_stage=True, cond_latent1=one)), None, 0, None) == bad  # one image latent of two
    assert plan(ctypes.byref(make(ltx, two_stage=True, cond_latent2=one)), None, 0, None) == bad
    assert plan(ctypes.byref(make(ltx)), None, -1, None) == bad
    assert plan(ctypes.byref(make(ltx)), None, 2, None) == bad  # room for two, nowhere to put them
    with pytest.raises(ltx.LTXError, match="at least 2"):
        ltx.dual_noise_plan(make(ltx, sigmas1=[1.0]))
