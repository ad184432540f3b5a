"""The audio text context (csrc/connector.cpp, ltx_connector_encode_av*): the feature extractor once, then the video
Embeddings1DConnector and a second, independently weighted one on its output (LTXTextEncoder.swift:628-636, :705-713). The small
connector configuration of tests/test_connector_gpu.py. Everything here is exact: the audio set runs the launches of the video set on
other weights, so its context is the context a connector loaded with those weights under the video names gives, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIM, HEADS, LAYERS, REGS, STATES = 256, 2, 2, 8, 5
VIDEO, AUDIO = "model.diffusion_model.video_embeddings_connector.", "model.diffusion_model.audio_embeddings_connector."


def file_tensors(oracle, w):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for k, v in oracle.connector_file_keys(w).items()}


def with_audio(video, audio):
    """The video file's tensors plus the connector tensors of `audio` under the audio names."""
    out = dict(video)
    out.update({AUDIO + k[len(VIDEO):]: v.clone() for k, v in audio.items() if k.startswith(VIDEO)})  # a file holds no shared tensors
    return out


@pytest.fixture(scope="module")
def env(ltx, oracle, tmp_path_factory):
    from safetensors.torch import save_file

    d = tmp_path_factory.mktemp("connector_av")
    wv = oracle.synth_connector_weights(dim=DIM, heads=HEADS, layers=LAYERS, registers=REGS, states=STATES, seed=3)
    wa = oracle.synth_connector_weights(dim=DIM, heads=HEADS, layers=LAYERS, registers=REGS, states=STATES, seed=4)
    tv, ta = file_tensors(oracle, wv), file_tensors(oracle, wa)
    ta_as_video = dict(tv)  # the audio set under the video names, behind the same feature extractor
    ta_as_video.update({k: v for k, v in ta.items() if k.startswith(VIDEO)})
    files = {"video_only": tv, "copy": with_audio(tv, tv), "different": with_audio(tv, ta), "audio_as_video": ta_as_video}
    for name, t in files.items():
        save_file(t, str(d / f"{name}.safetensors"))
    cfg = ltx.connector_config(dim=DIM, heads=HEADS, layers=LAYERS, registers=REGS, states=STATES)
    rng = np.random.default_rng(21)
    B, T = 2, 32
    hs = oracle.bf16_round((rng.standard_normal((STATES, B, T, DIM)) * 2.5 + 0.3).astype(np.float32))
    am = np.zeros((B, T), np.int32)
    am[0, T - 21:] = 1  # left padding: registers fill 11 and 27 positions
    am[1, T - 5:] = 1
    ctx = ltx.Context(0)
    yield {"ctx": ctx, "dir": d, "cfg": cfg, "hidden": oracle.f32_to_bf16_bits(hs), "mask": am, "n_video": len(tv)}
    ctx.close()


def encode(ctx, env, av):
    h = torch.from_numpy(env["hidden"].astype(np.int16)).cuda().view(torch.bfloat16)
    m = torch.from_numpy(env["mask"]).cuda()
    B, T = env["mask"].shape
    v = torch.zeros((B, T, DIM), device="cuda", dtype=torch.bfloat16)
    a = torch.zeros((B, T, DIM), device="cuda", dtype=torch.bfloat16)
    om = torch.zeros((B, T), device="cuda", dtype=torch.int32)
    if av:
        ctx.connector_encode_av_dev(h, m, v, a, om)
    else:
        ctx.connector_encode_dev(h, m, v, om)
    torch.cuda.synchronize()
    return v.view(torch.int16).cpu().numpy(), a.view(torch.int16).cpu().numpy(), om.cpu().numpy()


def test_a_copy_of_the_video_set_gives_the_video_context(env):
    ctx = env["ctx"]
    ctx.connector_load(env["dir"] / "copy.safetensors", env["cfg"])
    assert ctx.connector_has_audio()
    rep = ctx.load_report()  # the report stays the video set's
    assert rep["missing"] == 0 and rep["unmatched"] == 0 and rep["loaded"] == env["n_video"], rep
    v, a, om = encode(ctx, env, av=True)
    assert v.any() and np.array_equal(a, v) and om.all()


def test_a_different_audio_set_is_a_connector_of_its_own(env, ltx):
    ctx = env["ctx"]
    ctx.connector_load(env["dir"] / "different.safetensors", env["cfg"])
    v, a, om = encode(ctx, env, av=True)
    v_plain, _, om_plain = encode(ctx, env, av=False)
    assert np.array_equal(v, v_plain) and np.array_equal(om, om_plain) and om.all()  # the video context and the mask of the plain call
    assert not np.array_equal(a, v)
    other = ltx.Context(0)
    try:
        other.connector_load(env["dir"] / "audio_as_video.safetensors", env["cfg"])
        assert not other.connector_has_audio()
        want, _, _ = encode(other, env, av=False)
    finally:
        other.close()
    assert np.array_equal(a, want)
    # the host entry
    hv, ha, hm = ctx.connector_encode_av(env["hidden"], env["mask"])
    assert np.array_equal(hv.view(np.int16), v) and np.array_equal(ha.view(np.int16), a) and hm.all()
    hv2, _ = ctx.connector_encode(env["hidden"], env["mask"])
    assert np.array_equal(hv2.view(np.int16), v)


def test_without_an_audio_set_the_call_is_refused_and_the_file_loads_as_before(env, ltx):
    ctx = env["ctx"]
    ctx.connector_load(env["dir"] / "video_only.safetensors", env["cfg"])
    rep = ctx.load_report()
    assert rep["missing"] == 0 and rep["unmatched"] == 0 and rep["loaded"] == env["n_video"], rep
    assert not ctx.connector_has_audio()
    v_plain, _, _ = encode(ctx, env, av=False)
    assert v_plain.any()
    with pytest.raises(ltx.LTXError, match="audio embeddings connector") as e:
        encode(ctx, env, av=True)
    assert e.value.case == "modelNotLoaded"
    with pytest.raises(ltx.LTXError) as e:
        ctx.connector_encode_av(env["hidden"], env["mask"])
    assert e.value.case == "modelNotLoaded"
    # the video context does not depend on whether an audio set is loaded
    ctx.connector_load(env["dir"] / "different.safetensors", env["cfg"])
    v, _, _ = encode(ctx, env, av=False)
    assert np.array_equal(v, v_plain)
    ctx.connector_unload()
    assert not ctx.connector_has_audio()


def test_synthetic_weights_come_with_an_audio_set_of_their_own_seed(env):
    ctx = env["ctx"]
    ctx.connector_init_synthetic(env["cfg"], seed=91)
    assert ctx.connector_has_audio()
    v, a, _ = encode(ctx, env, av=True)
    v_plain, _, _ = encode(ctx, env, av=False)
    assert np.array_equal(v, v_plain) and a.any() and not np.array_equal(a, v)
    ctx.connector_unload()
