"""Model-slot lifecycle of the seven components through the C ABI: a slot of the context is either empty or a fully built model.

Only documented error returns are used: modelNotLoaded before a load, fileNotFound from a load, LTX_OK from an unload. The not-loaded
texts are the library's, per component (hosts and the mirrors may match on them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOT_LOADED, FILE_NOT_FOUND = 1, 9


def _bits(ltx, rng, shape):
    return ltx.f32_to_bf16_bits(rng.standard_normal(shape).astype(np.float32))


def _dit_cfg(ltx):
    return ltx.default_transformer_config(num_layers=2, num_attention_heads=4, cross_attention_dim=512, caption_channels=256)


def _conn_cfg(ltx):
    return ltx.connector_config(dim=256, heads=2, layers=2, registers=8, states=5)


def _run_dit(ltx, ctx):
    rng = np.random.default_rng(0)
    F, H, W, S = 2, 4, 4, 32
    return ctx.dit_forward(_bits(ltx, rng, (1, F * H * W, 128)), _bits(ltx, rng, (1, S, 256)), np.array([0.9], np.float32), None, F, H, W)


def _run_vae(ltx, ctx):
    return ctx.vae_decode(np.random.default_rng(1).standard_normal((1, 128, 2, 2, 2)).astype(np.float32))


def _run_upscaler(ltx, ctx):
    return ctx.upscale_latent(np.random.default_rng(2).standard_normal((1, 128, 1, 2, 2)).astype(np.float32))


def _run_connector(ltx, ctx):
    rng = np.random.default_rng(3)
    mask = np.zeros((1, 16), np.int32)
    mask[:, 5:] = 1  # left padding
    return ctx.connector_encode(_bits(ltx, rng, (5, 1, 16, 256)), mask)[0]


def _run_vae_encoder(ltx, ctx):
    return ctx.vae_encode(np.random.default_rng(4).uniform(-1, 1, (1, 3, 1, 32, 32)).astype(np.float32))


def _run_audio_vae(ltx, ctx):
    return ctx.audio_vae_decode(np.random.default_rng(5).standard_normal((8, 5, 16)).astype(np.float32))


def _run_vocoder(ltx, ctx):
    return ctx.vocoder_forward(np.random.default_rng(6).standard_normal((2, 9, 64)).astype(np.float32))


# name -> (not-loaded text, run, init_synthetic(ctx, seed) or None, load(ctx, path), unload)
COMPONENTS = {
    "transformer": ("Model component not loaded: transformer", _run_dit,
                    lambda ltx, c, seed: c.dit_init_synthetic(_dit_cfg(ltx), seed), lambda ltx, c, p: c.dit_load(p, _dit_cfg(ltx)),
                    lambda c: c.dit_unload()),
    "vae": ("Model component not loaded: vaeDecoder", _run_vae,
            lambda ltx, c, seed: c.vae_init_synthetic(seed), lambda ltx, c, p: c.vae_load(p), lambda c: c.vae_unload()),
    "upscaler": ("Model component not loaded: spatial upscaler", _run_upscaler,
                 None, lambda ltx, c, p: c.upscaler_load(p), lambda c: c.upscaler_unload()),
    "connector": ("Model not loaded: text-embedding connector", _run_connector,
                  lambda ltx, c, seed: c.connector_init_synthetic(_conn_cfg(ltx), seed),
                  lambda ltx, c, p: c.connector_load(p, _conn_cfg(ltx)), lambda c: c.connector_unload()),
    "vae_encoder": ("Model not loaded: VAE encoder failed to load", _run_vae_encoder,
                    lambda ltx, c, seed: c.vae_encoder_init_synthetic(64, seed), lambda ltx, c, p: c.vae_encoder_load(p, 64),
                    lambda c: c.vae_encoder_unload()),
    "audio_vae": ("Model not loaded: audio VAE not loaded", _run_audio_vae,
                  lambda ltx, c, seed: c.audio_vae_init_synthetic(32, seed), lambda ltx, c, p: c.audio_vae_load(p),
                  lambda c: c.audio_vae_unload()),
    "vocoder": ("Model not loaded: vocoder not loaded", _run_vocoder,
                lambda ltx, c, seed: c.vocoder_init_synthetic(128, seed), lambda ltx, c, p: c.vocoder_load(p),
                lambda c: c.vocoder_unload()),
}
SYNTHETIC = [n for n, c in COMPONENTS.items() if c[2] is not None]


@pytest.fixture()
def fresh_ctx(ltx):
    """A context of the test's own: nothing any other test loaded is in its slots."""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = ltx.Context(0)
    yield ctx
    ctx.close()


def _assert_not_loaded(ltx, ctx, name):
    text, run = COMPONENTS[name][:2]
    with pytest.raises(ltx.LTXError) as e:
        run(ltx, ctx)
    assert e.value.code == NOT_LOADED, (name, e.value)
    assert str(e.value) == f"LTXError.modelNotLoaded: {text}", (name, e.value)


@pytest.mark.parametrize("name", list(COMPONENTS))
def test_forward_before_load_reports_not_loaded(ltx, fresh_ctx, name):
    """Forward / decode / encode on an empty slot: LTX_ERR_MODEL_NOT_LOADED and the component's own text from ltx_last_error."""
    _assert_not_loaded(ltx, fresh_ctx, name)


@pytest.mark.parametrize("name", list(COMPONENTS))
def test_failed_load_leaves_the_slot_empty(ltx, fresh_ctx, tmp_path, name):
    """A load of a file that does not exist, after a successful init_synthetic (where the component has one), returns fileNotFound
    and leaves the slot empty: the next forward reports not-loaded, it does not run on the replaced or a half-built model."""
    init, load = COMPONENTS[name][2:4]
    if init is not None:
        init(ltx, fresh_ctx, 7)
    with pytest.raises(ltx.LTXError) as e:
        load(ltx, fresh_ctx, tmp_path / "no_such_file.safetensors")
    assert e.value.code == FILE_NOT_FOUND, (name, e.value)
    _assert_not_loaded(ltx, fresh_ctx, name)


@pytest.mark.parametrize("name", SYNTHETIC)
def test_init_twice_equals_init_once(ltx, fresh_ctx, name):
    """init_synthetic twice (the second replaces a live model), then one forward: bit-equal to a single init with the same seed on a
    context of its own."""
    run, init = COMPONENTS[name][1:3]
    init(ltx, fresh_ctx, 5)
    init(ltx, fresh_ctx, 11)
    twice = run(ltx, fresh_ctx)
    once_ctx = ltx.Context(0)
    try:
        init(ltx, once_ctx, 11)
        once = run(ltx, once_ctx)
    finally:
        once_ctx.close()
    assert twice.shape == once.shape
    if once.dtype != np.uint16:  # the connector returns bf16 bits
        assert np.isfinite(once).all()
    assert np.array_equal(twice, once), name


@pytest.mark.parametrize("name", list(COMPONENTS))
def test_unload_of_an_empty_slot_is_ok(ltx, fresh_ctx, name):
    """*_unload on an empty slot returns LTX_OK (the mirror raises on anything else), and the slot stays empty."""
    COMPONENTS[name][4](fresh_ctx)
    COMPONENTS[name][4](fresh_ctx)
    _assert_not_loaded(ltx, fresh_ctx, name)
