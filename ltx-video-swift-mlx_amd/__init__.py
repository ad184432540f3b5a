"""ltx-video-swift-mlx_amd - MI355X-native LTX-2 denoise + VAE-decode path.

The product is ``csrc/build/libltxhip.so`` (hand-written gfx950 HIP kernels behind the C ABI of
``include/ltxhip.h``). This Python package is the thin host-side mirror used by the test-suite and ``bench.py``:
``Context`` wraps an ``ltx_ctx``; device buffers are torch tensors used purely as HBM allocations (their
``data_ptr()`` is what crosses the ABI).

The directory name contains hyphens (it is the repo's mandated package name), so import it with
``importlib.import_module("ltx-video-swift-mlx_amd")`` - ``tests/conftest.py`` and ``bench.py`` do that and alias it
as ``ltx_amd``.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (ALLGATHER_FN, DIST_ID_BYTES, SHARD_CFG, SHARD_NONE, SHARD_SEQUENCE, ConnectorConfig, GemmaConfig, PROGRESS_CB, DenoiseOptions,
                   DualBlockConfig, DualDenoiseArgs, DualForwardArgs, DualGenerateArgs, NoiseDraw, NoiseJob, DualModelConfig, DualModelForwardArgs, DualRestageJob, DualStepJob, DualTwoStageArgs,
                   GemmTileLaunch, GemvJob, GemvJobQ, LTXError, NormMod2Job, TransformerConfig, lib)

__version__ = lib.ltx_version().decode()


def _check(rc, ctx=None):
    if rc != 0:
        msg = lib.ltx_last_error(ctx).decode(errors="replace") if True else ""
        raise LTXError(rc, msg)


def default_dual_block_config(**overrides):
    """``ltx_dual_block_config`` with the reference defaults (48 blocks, video 32 x 128, audio 32 x 64), fields overridden by keyword.
    ``video_heads`` / ``audio_heads`` given without their dims set ``video_dim`` = heads * 128 and ``audio_dim`` = heads * 64, and the
    context dims follow the stream dims unless given."""
    cfg = DualBlockConfig()
    lib.ltx_dual_block_config_default(C.byref(cfg))
    o = dict(overrides)
    if "video_heads" in o:
        o.setdefault("video_dim", o["video_heads"] * 128)
    if "audio_heads" in o:
        o.setdefault("audio_dim", o["audio_heads"] * 64)
    if "video_dim" in o:
        o.setdefault("video_context_dim", o["video_dim"])
    if "audio_dim" in o:
        o.setdefault("audio_context_dim", o["audio_dim"])
    for k, v in o.items():
        if k == "max_pos":
            for i in range(3):
                cfg.max_pos[i] = v[i]
        else:
            getattr(cfg, k)
            setattr(cfg, k, v)
    return cfg


def default_dual_model_config(**overrides):
    """``ltx_dual_model_config`` with the reference defaults. Keywords that name a field of the block config (``num_layers``,
    ``video_heads``, ...) go to ``default_dual_block_config``; the others (``in_channels``, ``caption_channels``, ...) are set here."""
    cfg = DualModelConfig()
    lib.ltx_dual_model_config_default(C.byref(cfg))
    block_fields = {f[0] for f in DualBlockConfig._fields_}
    cfg.blocks = default_dual_block_config(**{k: v for k, v in overrides.items() if k in block_fields})
    for k, v in overrides.items():
        if k not in block_fields:
            getattr(cfg, k)
            setattr(cfg, k, v)
    return cfg


def default_transformer_config(**overrides):
    cfg = TransformerConfig()
    lib.ltx_transformer_config_default(C.byref(cfg))
    for k, v in overrides.items():
        if k == "max_pos":
            for i in range(3):
                cfg.max_pos[i] = v[i]
        else:
            setattr(cfg, k, v)
    return cfg


# ---------------------------------------------------------------------------------------------------------------
# pure-host helpers (no GPU)
# ---------------------------------------------------------------------------------------------------------------
def validate_generation_config(width, height, num_frames, num_steps, cfg_scale, two_stage=False):
    """``LTXVideoGenerationConfig.validate()``: raises LTXError.invalidConfiguration with the reference's text."""
    buf = C.create_string_buffer(256)
    rc = lib.ltx_validate_generation_config(width, height, num_frames, num_steps, cfg_scale, int(two_stage), buf, 256)
    if rc != 0:
        raise LTXError(rc, buf.value.decode())


def latent_shape(width, height, num_frames):
    f, h, w = C.c_int(), C.c_int(), C.c_int()
    _check(lib.ltx_latent_shape(width, height, num_frames, C.byref(f), C.byref(h), C.byref(w)))
    return f.value, h.value, w.value


def sigmas(distilled, num_steps, token_count=0):
    out = (C.c_float * 128)()
    n = lib.ltx_sigmas(int(distilled), num_steps, token_count or 0, out, 128)
    if n < 0:
        raise LTXError(-n, "invalid sigma request")
    return np.array(out[:n], dtype=np.float32)


def stage2_sigmas():
    out = (C.c_float * 4)()
    lib.ltx_stage2_sigmas(out, 4)
    return np.array(out[:], dtype=np.float32)


def rope_tables(cfg, F, H, W):
    D = cfg.num_attention_heads * cfg.attention_head_dim
    T = F * H * W
    cos = np.empty((T, D // 2), dtype=np.float32)
    sin = np.empty((T, D // 2), dtype=np.float32)
    _check(lib.ltx_rope_tables(C.byref(cfg), F, H, W, cos.ctypes.data, sin.ctypes.data))
    return cos, sin


def vae_tile_plan(latent_frames, tile, overlap):
    starts, ends = (C.c_int * 256)(), (C.c_int * 256)()
    out = C.c_int()
    n = lib.ltx_vae_tile_plan(latent_frames, tile, overlap, starts, ends, 256, C.byref(out))
    if n < 0:
        raise LTXError(-n, "invalid tiling request")
    return [(starts[i], ends[i]) for i in range(n)], out.value


def _map_key(fn, key):
    buf = C.create_string_buffer(1024)
    rc = fn(key.encode(), buf, 1024)
    if rc < 0:
        raise LTXError(2, "key too long")
    return buf.value.decode() if rc == 1 else None


def map_transformer_key(key):
    return _map_key(lib.ltx_map_transformer_key, key)


def map_vae_key(key):
    return _map_key(lib.ltx_map_vae_key, key)


def map_lora_key(key):
    return _map_key(lib.ltx_map_lora_key, key)


def mlx_random_normal(seed, shape, draw_index=0):
    """MLXRandom.seed(seed); MLXRandom.normal(shape) - the reference's generateNoise (LatentUtils.swift:69-83), restated."""
    out = np.empty(shape, np.float32)
    _check(lib.ltx_mlx_random_normal(int(seed), int(draw_index), out.ctypes.data, out.size))
    return out


def mlx_draw_key(seed, draw_index=0):
    """``ltx_mlx_draw_key``: the two uint32 key words of the draw_index-th keyless draw after MLXRandom.seed(seed)."""
    o = np.empty(2, np.uint32)
    _check(lib.ltx_mlx_draw_key(int(seed), int(draw_index), o.ctypes.data_as(C.POINTER(C.c_uint32))))
    return o


NOISE_ROLES = ("VIDEO1", "AUDIO1", "COND1", "VIDEO2", "AUDIO2", "COND2")


def dual_generate_args(seed, F, H, W, T_a, S, sigmas1, two_stage=False, sigmas2=None, channels=128, video_latent=None, audio_latent=None,
                       video_context=None, audio_context=None, mask=None, cfg_scale=1.0, guidance_rescale=0.0, cond_latent1=None,
                       cond_latent2=None, image_cond_noise_scale=0.0, noise_workspace=None, stage1_out=None, struct_size=None):
    """A filled ``ltx_dual_generate_args``. Tensors / arrays are passed by pointer; the struct keeps them (and the sigma arrays) alive."""
    a = DualGenerateArgs()
    a.struct_size = C.sizeof(DualGenerateArgs) if struct_size is None else struct_size
    a.two_stage, a.seed, a.channels = int(bool(two_stage)), int(seed), channels
    a.F, a.H, a.W, a.T_a, a.S = F, H, W, T_a, S
    keep = [video_latent, audio_latent, video_context, audio_context, mask, cond_latent1, cond_latent2, noise_workspace, stage1_out]
    a.video_latent, a.audio_latent = _ptr(video_latent), _ptr(audio_latent)
    if sigmas1 is not None:
        sg1 = np.ascontiguousarray(sigmas1, dtype=np.float32)
        a.sigmas1, a.n_sigmas1 = sg1.ctypes.data_as(C.POINTER(C.c_float)), len(sg1)
        keep.append(sg1)
    if sigmas2 is not None:
        sg2 = np.ascontiguousarray(sigmas2, dtype=np.float32)
        a.sigmas2, a.n_sigmas2 = sg2.ctypes.data_as(C.POINTER(C.c_float)), len(sg2)
        keep.append(sg2)
    a.video_context, a.audio_context, a.mask = _ptr(video_context), _ptr(audio_context), _ptr(mask)
    a.cfg_scale, a.guidance_rescale = cfg_scale, guidance_rescale
    a.cond_latent1, a.cond_latent2, a.image_cond_noise_scale = _ptr(cond_latent1), _ptr(cond_latent2), image_cond_noise_scale
    a.noise_workspace, a.stage1_out = _ptr(noise_workspace), _ptr(stage1_out)
    a._keep = keep
    return a


def dual_noise_plan(args, cap=None):
    """``ltx_dual_noise_plan``: (list of dicts(draw_index, role, step, numel, offset, scale), total_floats). ``cap`` smaller than the
    number of draws returns (count, total_floats) instead, as the C call does."""
    total = C.c_long(0)
    n = lib.ltx_dual_noise_plan(C.byref(args) if args is not None else None, None, 0, C.byref(total))
    if n < 0:
        _check(-n)
    if cap is not None and cap < n:
        arr = (NoiseDraw * max(cap, 1))()
        return lib.ltx_dual_noise_plan(C.byref(args), arr, cap, C.byref(total)), total.value
    arr = (NoiseDraw * max(n, 1))()
    n = lib.ltx_dual_noise_plan(C.byref(args), arr, n, C.byref(total))
    return [dict(draw_index=d.draw_index, role=d.role, step=d.step, numel=d.numel, offset=d.offset, scale=d.scale) for d in arr[:n]], total.value


def threefry2x32(key, ctr):
    k = np.asarray(key, np.uint32)
    c = np.asarray(ctr, np.uint32)
    o = np.empty(2, np.uint32)
    lib.ltx_threefry2x32(k.ctypes.data, c.ctypes.data, o.ctypes.data)
    return o




def set_option(key, value):
    """``ltx_ctx_set_option`` without a context: the launchers' switch table is process-wide (csrc/options.h)."""
    _check(lib.ltx_ctx_set_option(None, key.encode(), int(value)))


def get_option(key):
    v = C.c_int()
    _check(lib.ltx_ctx_get_option(None, key.encode(), C.byref(v)))
    return v.value


def conv_takes_d2s_pn(F, H, W, C):
    """``ltx_conv_takes_d2s_pn``: does the decoder's upsampler conv C -> 4C at (F, H, W) carry the next stage's first PixelNorm?"""
    return bool(lib.ltx_conv_takes_d2s_pn(F, H, W, C))


def gemm_dense_tile_cfg(M, N, K, act=0, flags=2, ncu=256):
    """``ltx_gemm_dense_tile_cfg``: the tile configuration the launcher picks for a dense GEMM launch on a device of ``ncu`` CUs."""
    return lib.ltx_gemm_dense_tile_cfg(M, N, K, act, flags, ncu)


def option_table():
    """[(name, default, min, max, numerics, doc)] of every switch (``ltx_option_info``)."""
    n = lib.ltx_option_info(-1, None, None, None, None, None, None)
    out = []
    for i in range(n):
        name, doc = C.c_char_p(), C.c_char_p()
        d, lo, hi, num = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib.ltx_option_info(i, C.byref(name), C.byref(d), C.byref(lo), C.byref(hi), C.byref(num), C.byref(doc))
        out.append((name.value.decode(), d.value, lo.value, hi.value, bool(num.value), doc.value.decode()))
    return out


@contextlib.contextmanager
def options(**kv):
    """Set switches for the duration of a ``with`` block and restore the previous values (tests, A/B runs)."""
    old = {k: get_option(k) for k in kv}
    try:
        for k, v in kv.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


def dist_unique_id():
    """``ltx_dist_unique_id``: the 128 bytes one rank creates and the host carries to the others (RCCL's ncclUniqueId)."""
    buf = C.create_string_buffer(DIST_ID_BYTES)
    _check(lib.ltx_dist_unique_id(buf))
    return buf.raw


class _Transport:
    """Python all-gather behind ``ltx_allgather_fn``. ctypes would print and swallow an exception raised inside a callback and the
    C side would carry on with unfilled buffers: here the exception is stashed, the callback returns 1 (the library aborts the call
    with LTX_ERR_GENERATION_FAILED) and ``reraise`` surfaces the original error once the C call has returned."""

    def __init__(self, gather):
        self.error = None

        def _cb(_user, send, recv, nbytes):
            try:
                gather(send, recv, nbytes)
                return 0
            except BaseException as e:  # noqa: BLE001 - must not propagate through the C frames
                self.error = e
                return 1

        self.cfn = ALLGATHER_FN(_cb)

    def reraise(self):
        if self.error is not None:
            e, self.error = self.error, None
            raise e


def frames_to_u8(frames):
    """``VideoExporter.tensorToImages`` pixel conversion: uint8(clip(x,0,1)*255), truncating."""
    f = np.ascontiguousarray(frames, dtype=np.float32)
    out = np.empty(f.shape, dtype=np.uint8)
    _check(lib.ltx_frames_to_u8(f.ctypes.data, f.size, out.ctypes.data))
    return out


def write_png(path, rgb):
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, c = a.shape
    assert c == 3
    _check(lib.ltx_write_png(str(path).encode(), a.ctypes.data, w, h))


def audio_latent_frames(video_frames, fps=24.0):
    """``computeAudioLatentFrames`` (LTXPipeline.swift:530-534)."""
    return lib.ltx_audio_latent_frames(int(video_frames), float(fps))


def audio_mel_frames(T):
    return lib.ltx_audio_mel_frames(int(T))


def audio_sample_count(T):
    return lib.ltx_audio_sample_count(int(T))


def audio_sample_rate():
    return lib.ltx_audio_sample_rate()


def write_wav(path, waveform, sample_rate=None, gain=1.0):
    """``AudioExporter.exportToWAV``: waveform (2, n) f32 -> 16-bit stereo PCM file."""
    a = np.ascontiguousarray(waveform, dtype=np.float32)
    assert a.ndim == 2 and a.shape[0] == 2
    _check(lib.ltx_write_wav(str(path).encode(), a.ctypes.data, a.shape[1], int(sample_rate or audio_sample_rate()), float(gain)))


def map_vae_encoder_key(key):
    """``mapVAEEncoderWeights`` (ModelDownloader.swift:1222-1283); None for non-encoder tensors."""
    return _map_key(lib.ltx_map_vae_encoder_key, key)


def vae_encoder_latent_frames(T):
    return lib.ltx_vae_encoder_latent_frames(T)


def map_text_encoder_key(key):
    """``mapTextEncoderWeights`` (ModelDownloader.swift:911-968); None = dropped."""
    return _map_key(lib.ltx_map_text_encoder_key, key)


def connector_config(**kw):
    cfg = ConnectorConfig()
    lib.ltx_connector_config_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def gemma_config(**kw):
    """``ltx_gemma_config`` with the reference's ``Gemma3Config`` defaults, fields overridden by keyword."""
    cfg = GemmaConfig()
    lib.ltx_gemma_config_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def lm_params(**kw):
    """``ltx_lm_params`` with the reference's ``generateTokens`` defaults (512 new tokens, temperature 0.7, top_p 0.95, penalty 1.1,
    context 64, eos {1}); fields overridden by keyword. ``eos_ids`` may be given as a list of up to 8 ids (sets ``n_eos`` too)."""
    p = _lib.LmParams()
    lib.ltx_lm_params_default(C.byref(p))
    eos = kw.pop("eos_ids", None)
    for k, v in kw.items():
        setattr(p, k, v)
    if eos is not None:
        eos = [int(e) for e in eos]
        if len(eos) > 8:
            raise ValueError("up to 8 stop ids")
        p.n_eos = len(eos)
        for i, e in enumerate(eos):
            p.eos_ids[i] = e
    return p


def lm_sample_host(logits, generated=(), context=64, penalty=1.1, temperature=0.7, top_p=0.95, seed=0, step=0):
    """``ltx_lm_sample_host``: this library's sampler, pure host code. ``logits`` is a float32 numpy array that the repetition penalty
    rewrites IN PLACE; returns the token."""
    assert isinstance(logits, np.ndarray) and logits.dtype == np.float32 and logits.flags["C_CONTIGUOUS"]
    gen = np.ascontiguousarray(generated, dtype=np.int32)
    tok = C.c_int32()
    _check(lib.ltx_lm_sample_host(logits.ctypes.data, logits.size, gen.ctypes.data if gen.size else None, gen.size, context, penalty, temperature,
                                  top_p, seed, step, C.byref(tok)))
    return tok.value


def gemv_bf16_rows_per_workgroup(N, epilogue=0):
    return int(lib.ltx_gemv_bf16_rows_per_workgroup(N, epilogue))


def rope_tables_1d(T, dim=3840, theta=10000.0, max_pos=4096):
    cos = np.empty((T, dim // 2), dtype=np.float32)
    sin = np.empty((T, dim // 2), dtype=np.float32)
    _check(lib.ltx_rope_tables_1d(T, dim, theta, max_pos, cos.ctypes.data, sin.ctypes.data))
    return cos, sin


def audio_positions(T_a):
    """``createAudioPositionGrid`` (LTXRoPE.swift:627-655): seconds of the middle of each audio latent frame, f32 [T_a]."""
    out = np.empty(int(T_a), dtype=np.float32)
    _check(lib.ltx_audio_positions(int(T_a), out.ctypes.data))
    return out


def video_temporal_positions(F, H, W, fps=24.0):
    """Row 0 of ``createPositionGrid``: the temporal coordinate of every video token in token order, f32 [F*H*W]."""
    out = np.empty(F * H * W, dtype=np.float32)
    _check(lib.ltx_video_temporal_positions(F, H, W, float(fps), out.ctypes.data))
    return out


def rope_tables_positions(positions, dim, theta=10000.0, max_pos=20):
    """``precomputeFreqsCis`` (f64 path) over one real-valued position per token: cos, sin [T][dim/2] f32."""
    pos = np.ascontiguousarray(positions, dtype=np.float32)
    cos = np.empty((pos.size, dim // 2), dtype=np.float32)
    sin = np.empty((pos.size, dim // 2), dtype=np.float32)
    _check(lib.ltx_rope_tables_positions(pos.ctypes.data, pos.size, dim, theta, max_pos, cos.ctypes.data, sin.ctypes.data))
    return cos, sin


ATTN_QUERY_PRESCALE_64 = float(np.float32(0.125) * np.float32(1.4426950408889634))  # csrc/attention.h kAttnQueryPrescale64


# ---------------------------------------------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------------------------------------------
def timestep_groups(token_timesteps):
    """Per-token timesteps [B][T] -> (ts [B][G] f32, row_map [B*T] int32) for ``dual_model_forward_groups_dev``: the distinct values of
    each batch element in order of first appearance (as ``ltx_dit_forward_tokens`` groups them), G = the largest count, unused slots
    repeat the element's first value; row_map[b*T + t] = b*G + group(b, t). More than 8 rows in all (B * G > 8) is refused."""
    tt = np.ascontiguousarray(token_timesteps, dtype=np.float32)
    if tt.ndim != 2 or tt.shape[0] < 1 or tt.shape[1] < 1:
        raise ValueError("timestep_groups: token_timesteps must be [B][T]")
    B, T = tt.shape
    values, groups = [], np.zeros((B, T), np.int32)
    for b in range(B):
        vals = []
        for t in range(T):
            v = tt[b, t]
            for g, u in enumerate(vals):
                if u == v:
                    break
            else:
                g = len(vals)
                vals.append(v)
                if B * len(vals) > 8:
                    raise ValueError(f"timestep_groups: more than {8 // B} distinct timesteps in batch element {b} (B * G <= 8)")
            groups[b, t] = g
        values.append(vals)
    G = max(len(v) for v in values)
    ts = np.stack([np.array(v + [v[0]] * (G - len(v)), np.float32) for v in values])
    row_map = (groups + (np.arange(B, dtype=np.int32) * G)[:, None]).astype(np.int32).reshape(-1)
    return ts, row_map


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    assert t.is_contiguous()
    return t.data_ptr()


def _dptr(t):
    """Address of a device tensor's first element (None -> NULL); the tensor may be a view at an offset into a longer one."""
    return None if t is None else t.data_ptr()


def fe_stats_partials_floats(states, B, T, D):
    """f32 elements of scratch that ``Context.op_fe_stats`` needs for this shape."""
    return int(lib.ltx_fe_stats_partials_floats(states, B, T, D))


class Context:
    """Owns an ``ltx_ctx``. All ``*_dev`` methods take torch tensors resident on this context's GPU."""

    def __init__(self, device=0, use_torch_stream=True):
        h = C.c_void_p()
        rc = lib.ltx_ctx_create(device, C.byref(h))
        if rc != 0:
            raise LTXError(rc, lib.ltx_last_error(None).decode(errors="replace"))
        self._h = h
        self.device = device
        if use_torch_stream:
            import torch

            self.set_stream(torch.cuda.current_stream(device).cuda_stream)

    def close(self):
        if self._h:
            lib.ltx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        tr = getattr(self, "_transport", None)
        if tr is not None:
            tr.reraise()
        if rc != 0:
            raise LTXError(rc, lib.ltx_last_error(self._h).decode(errors="replace"))

    # ---- multi-GPU group of this context (include/ltxhip.h, "Multi-GPU") ----
    def dist_init(self, rank, world, unique_id):
        """RCCL communicator over the group's ranks (collective call); ``unique_id`` from ``dist_unique_id()`` on one rank."""
        assert len(unique_id) == DIST_ID_BYTES
        self._transport = None
        self._ck(lib.ltx_dist_init(self._h, rank, world, C.c_char_p(bytes(unique_id))))

    def dist_set_transport(self, rank, world, gather):
        """Same membership over a Python all-gather ``gather(send_ptr, recv_ptr, nbytes)`` (tests over gloo)."""
        self._transport = None
        tr = _Transport(gather)
        self._ck(lib.ltx_dist_set_transport(self._h, rank, world, C.cast(tr.cfn, C.c_void_p), None))
        self._transport = tr

    def dist_shutdown(self):
        self._transport = None
        self._ck(lib.ltx_dist_shutdown(self._h))

    def dist_info(self):
        r, w, nat, n = C.c_int(), C.c_int(), C.c_int(), C.c_long()
        self._ck(lib.ltx_dist_info(self._h, C.byref(r), C.byref(w), C.byref(nat), C.byref(n)))
        return {"rank": r.value, "world": w.value, "native": bool(nat.value), "collectives": n.value}

    def dist_allgather_dev(self, send, recv):
        self._ck(lib.ltx_dist_allgather_dev(self._h, _ptr(send), _ptr(recv), send.numel() * send.element_size()))

    def dist_broadcast_dev(self, buf, root=0):
        self._ck(lib.ltx_dist_broadcast_dev(self._h, _ptr(buf), buf.numel() * buf.element_size(), root))

    def dit_export_param(self, key):
        """One resident parameter as an f32 numpy array (flat), e.g. to hand the synthetic weights to the oracle."""
        n = lib.ltx_dit_export_param(self._h, key.encode(), None, 0)
        if n < 0:
            raise LTXError(-n, lib.ltx_last_error(self._h).decode(errors="replace"))
        out = np.empty(n, dtype=np.float32)
        n2 = lib.ltx_dit_export_param(self._h, key.encode(), out.ctypes.data, n)
        if n2 < 0:
            raise LTXError(-n2, lib.ltx_last_error(self._h).decode(errors="replace"))
        return out

    def set_option(self, key, value):
        """``ltx_ctx_set_option``: move one of the launchers' switches (process-wide; the library never reads the environment)."""
        self._ck(lib.ltx_ctx_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int()
        self._ck(lib.ltx_ctx_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def options(self, **kv):
        """``with ctx.options(qk_f32=1): ...`` - set for the block, restore afterwards (the table is process-wide)."""
        return options(**kv)

    def set_stream(self, stream_handle):
        self._ck(lib.ltx_ctx_set_stream(self._h, C.c_void_p(stream_handle)))

    def synchronize(self):
        self._ck(lib.ltx_ctx_synchronize(self._h))

    def load_report(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._ck(lib.ltx_load_report(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"loaded": a.value, "missing": b.value, "unmatched": c.value}

    # ---- DiT ----
    def dit_load(self, path, cfg=None, quant_bits=16, group_size=64):
        self._ck(lib.ltx_dit_load(self._h, str(path).encode(), C.byref(cfg) if cfg is not None else None, quant_bits, group_size))

    def dit_init_synthetic(self, cfg=None, seed=1234):
        self._ck(lib.ltx_dit_init_synthetic(self._h, C.byref(cfg) if cfg is not None else None, seed))

    def dit_quantize(self, bits, group_size=64):
        self._ck(lib.ltx_dit_quantize(self._h, bits, group_size))

    def dit_memory_info(self):
        v = [C.c_long() for _ in range(4)]
        self._ck(lib.ltx_dit_memory_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("bf16_weights", "quantised_weights", "scratch", "other"), (x.value for x in v)))

    def fuse_lora(self, path, scale=1.0):
        """``LTXPipeline.fuseLoRA(from:scale:)`` -> number of fused layers."""
        n = C.c_int()
        self._ck(lib.ltx_dit_fuse_lora(self._h, str(path).encode(), scale, C.byref(n)))
        return n.value

    def dit_unload(self):
        self._ck(lib.ltx_dit_unload(self._h))

    def dit_forward(self, latent_bf16, context_bf16, timesteps, mask, F, H, W):
        """Host-pointer path. latent [B,T,C] / context [B,S,Cc] as uint16 bf16 bit arrays, returns f32 [B,T,Cout]."""
        B, T, _ = latent_bf16.shape
        S = context_bf16.shape[1]
        assert T == F * H * W
        out_c = self._out_channels if hasattr(self, "_out_channels") else latent_bf16.shape[2]
        vel = np.empty((B, T, out_c), dtype=np.float32)
        ts = np.ascontiguousarray(timesteps, dtype=np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        self._ck(lib.ltx_dit_forward(self._h, _ptr(np.ascontiguousarray(latent_bf16)), _ptr(np.ascontiguousarray(context_bf16)),
                                     _ptr(ts), _ptr(m), B, F, H, W, S, _ptr(vel)))
        return vel

    def dit_forward_tokens(self, latent_bf16, context_bf16, token_timesteps, mask, F, H, W):
        """Per-token timesteps [B,T] (image-to-video, ``prepareTimestep``); otherwise as ``dit_forward``."""
        B, T, _ = latent_bf16.shape
        S = context_bf16.shape[1]
        assert T == F * H * W
        vel = np.empty((B, T, latent_bf16.shape[2]), dtype=np.float32)
        ts = np.ascontiguousarray(token_timesteps, dtype=np.float32)
        assert ts.shape == (B, T)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        self._ck(lib.ltx_dit_forward_tokens(self._h, _ptr(np.ascontiguousarray(latent_bf16)), _ptr(np.ascontiguousarray(context_bf16)),
                                            _ptr(ts), _ptr(m), B, F, H, W, S, _ptr(vel)))
        return vel

    def dit_forward_dev(self, latent, context, timesteps, mask, F, H, W, velocity, ctx_version=0, mask_all_ones=False):
        B, T = latent.shape[0], latent.shape[1]
        S = context.shape[1]
        self._ck(lib.ltx_dit_forward_dev(self._h, _ptr(latent), _ptr(context), _ptr(timesteps), _ptr(mask),
                                         int(mask_all_ones), B, F, H, W, S, ctx_version, _ptr(velocity)))

    def dit_forward_sp_dev(self, latent, context, timesteps, mask, F, H, W, velocity, sp_rank, sp_world, gather, ctx_version=0,
                           mask_all_ones=False):
        """Sequence-parallel forward: `latent` [1,Tn,C] / `velocity` [1,Tn,C] hold this rank's token slice; `gather(send_ptr,
        recv_ptr, nbytes)` all-gathers device memory over the ranks (see dist.sp_allgather_fn). Device tensors."""
        S = context.shape[1]
        tr = _Transport(gather) if gather is not None else None  # None: the context's own transport (dist_init / dist_set_transport)
        rc = lib.ltx_dit_forward_sp_dev(self._h, _ptr(latent), _ptr(context), _ptr(timesteps), _ptr(mask), int(mask_all_ones),
                                        F, H, W, S, ctx_version, sp_rank, sp_world, C.cast(tr.cfn, C.c_void_p) if tr else None, None,
                                        _ptr(velocity))
        if tr:
            tr.reraise()
        self._ck(rc)

    def dit_set_cross_attn_scale(self, scale, first=0, last=-1):
        self._ck(lib.ltx_dit_set_cross_attn_scale(self._h, scale, first, last))

    def dit_set_stg(self, blocks, skip_self_attention=True, skip_feed_forward=False):
        arr = (C.c_int * len(blocks))(*blocks)
        self._ck(lib.ltx_dit_set_stg(self._h, arr, len(blocks), int(skip_self_attention), int(skip_feed_forward)))

    def dit_clear_stg(self):
        self._ck(lib.ltx_dit_clear_stg(self._h))

    # ---- VAE ----
    def vae_load(self, path, config_json=None):
        self._ck(lib.ltx_vae_load(self._h, str(path).encode(), str(config_json).encode() if config_json else None))

    def vae_init_synthetic(self, seed=77, timestep_conditioning=False):
        self._ck(lib.ltx_vae_init_synthetic(self._h, seed, int(timestep_conditioning)))

    def vae_unload(self):
        self._ck(lib.ltx_vae_unload(self._h))

    @property
    def vae_timestep_conditioning(self):
        r = lib.ltx_vae_timestep_conditioning(self._h)
        if r < 0:
            raise LTXError(-r, "Model component not loaded: vaeDecoder")
        return bool(r)

    def vae_decode(self, latent, timestep=None, noise=None, tile=0, overlap=1):
        """Host path: latent [1,128,F,H,W] f32 -> frames (n,32H,32W,3) f32 in [0,1] (decodeVideo)."""
        lat = np.ascontiguousarray(latent, dtype=np.float32)
        _, _, F, H, W = lat.shape
        _, nf = vae_tile_plan(F, tile, overlap)
        out = np.empty((nf, H * 32, W * 32, 3), dtype=np.float32)
        n = C.c_int()
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
        self._ck(lib.ltx_vae_decode(self._h, _ptr(lat), F, H, W, int(timestep is not None), float(timestep or 0.0), _ptr(nz),
                                    tile, overlap, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    def vae_decode_dev(self, latent, F, H, W, frames, timestep=None, noise=None, tile=0, overlap=1):
        n = C.c_int()
        self._ck(lib.ltx_vae_decode_dev(self._h, _ptr(latent), F, H, W, int(timestep is not None), float(timestep or 0.0),
                                        _ptr(noise), tile, overlap, _ptr(frames), frames.numel(), C.byref(n)))
        return n.value

    def vae_decode_sharded_dev(self, latent, F, H, W, frames, timestep=None, noise=None, tile=0, overlap=1):
        """Tiles round-robin over the context's group, raw tiles broadcast, blend + clip on every rank."""
        n = C.c_int()
        self._ck(lib.ltx_vae_decode_sharded_dev(self._h, _ptr(latent), F, H, W, int(timestep is not None), float(timestep or 0.0),
                                                _ptr(noise), tile, overlap, _ptr(frames), frames.numel(), C.byref(n)))
        return n.value

    def vae_decode_gathered_dev(self, latent, F, H, W, frames, root=0, timestep=None, noise=None, tile=0, overlap=1):
        """Tiles decoded round-robin by the group's ranks, raw tiles sent to `root` only, which blends; frames=None elsewhere."""
        n = C.c_int()
        self._ck(lib.ltx_vae_decode_gathered_dev(self._h, _ptr(latent), F, H, W, int(timestep is not None), float(timestep or 0.0),
                                                 _ptr(noise), tile, overlap, root, _ptr(frames), 0 if frames is None else frames.numel(), C.byref(n)))
        return n.value

    def vae_decode_tile_dev(self, latent, F, H, W, tile, overlap, tile_index, out, timestep=None, noise=None):
        """RAW frames (pre-blend, pre-clip) of one tile of the plan -> out; returns its frame count."""
        n = C.c_int()
        self._ck(lib.ltx_vae_decode_tile_dev(self._h, _ptr(latent), F, H, W, int(timestep is not None), float(timestep or 0.0),
                                             _ptr(noise), tile, overlap, tile_index, _ptr(out), out.numel(), C.byref(n)))
        return n.value

    def vae_res_block_dev(self, group, block, x, F, H, W):
        """One res-block of the loaded decoder on the channels-last f32 stream x [F][H][W][C], in place."""
        self._ck(lib.ltx_vae_res_block_dev(self._h, group, block, _ptr(x), F, H, W))

    def vae_upsample_dev(self, group, x, F, H, W, out):
        """One depth-to-space upsampler of the loaded decoder: x [F][H][W][C] f32 -> out [2F-1][2H][2W][C/2] f32 (device tensors)."""
        self._ck(lib.ltx_vae_upsample_dev(self._h, group, _ptr(x), F, H, W, _ptr(out)))

    def vae_blend_tiles_dev(self, tiles, tile_frames, overlap, H, W, frames):
        n = C.c_int()
        ptrs = (C.c_void_p * len(tiles))(*[t.data_ptr() for t in tiles])
        nfs = (C.c_int * len(tiles))(*tile_frames)
        self._ck(lib.ltx_vae_blend_tiles_dev(self._h, ptrs, nfs, len(tiles), overlap, H, W, _ptr(frames), frames.numel(), C.byref(n)))
        return n.value

    def op_conv3d(self, x, w, bias, out, causal=False):
        F, H, W, Cin = x.shape
        Cout = w.shape[0]
        self._ck(lib.ltx_op_conv3d(self._h, _ptr(x), F, H, W, Cin, _ptr(w), _ptr(bias), Cout, int(causal), _ptr(out)))

    # ---- two-stage glue ----
    # ---- VAE encoder ----
    def vae_encoder_load(self, path, channel_base=0):
        self._ck(lib.ltx_vae_encoder_load(self._h, str(path).encode(), channel_base))

    def vae_encoder_init_synthetic(self, channel_base=0, seed=66):
        self._ck(lib.ltx_vae_encoder_init_synthetic(self._h, channel_base, seed))

    def vae_encoder_unload(self):
        self._ck(lib.ltx_vae_encoder_unload(self._h))

    def vae_encode(self, pixels, normalize=False):
        """``encodeImage`` without the image I/O: pixels [1,3,T,H,W] f32 -> latent [1,128,T',H/32,W/32] f32 (host arrays)."""
        px = np.ascontiguousarray(pixels, dtype=np.float32)
        _, _, T, H, W = px.shape
        out = np.empty((1, 128, lib.ltx_vae_encoder_latent_frames(T), H // 32, W // 32), dtype=np.float32)
        self._ck(lib.ltx_vae_encode(self._h, _ptr(px), T, H, W, int(normalize), _ptr(out)))
        return out

    def vae_encode_dev(self, pixels, latent, normalize=False):
        _, _, T, H, W = pixels.shape
        self._ck(lib.ltx_vae_encode_dev(self._h, _ptr(pixels), T, H, W, int(normalize), _ptr(latent)))

    # ---- audio decode leg (audio VAE decoder + vocoder) ----
    def audio_vae_load(self, path):
        self._ck(lib.ltx_audio_vae_load(self._h, str(path).encode()))

    def audio_vae_init_synthetic(self, base_channels=0, seed=55):
        self._ck(lib.ltx_audio_vae_init_synthetic(self._h, base_channels, seed))

    def audio_vae_unload(self):
        self._ck(lib.ltx_audio_vae_unload(self._h))

    def vocoder_load(self, path):
        self._ck(lib.ltx_vocoder_load(self._h, str(path).encode()))

    def vocoder_init_synthetic(self, hidden_channels=0, seed=56):
        self._ck(lib.ltx_vocoder_init_synthetic(self._h, hidden_channels, seed))

    def vocoder_unload(self):
        self._ck(lib.ltx_vocoder_unload(self._h))

    def audio_vae_decode(self, latent):
        """``AudioVAE.decode``: latent (8, T, 16) f32 -> mel (2, max(4T-3, 1), 64) f32 (host arrays)."""
        lat = np.ascontiguousarray(latent, dtype=np.float32)
        assert lat.shape[0] == 8 and lat.shape[2] == 16
        T = lat.shape[1]
        mel = np.empty((2, audio_mel_frames(T), 64), dtype=np.float32)
        self._ck(lib.ltx_audio_vae_decode(self._h, _ptr(lat), T, _ptr(mel)))
        return mel

    def audio_vae_decode_dev(self, latent, mel):
        self._ck(lib.ltx_audio_vae_decode_dev(self._h, _ptr(latent), latent.shape[1], _ptr(mel)))

    def vocoder_forward(self, mel):
        """``LTX2Vocoder``: mel (2, T, 64) f32 -> waveform (2, 240 T) f32 (host arrays)."""
        m = np.ascontiguousarray(mel, dtype=np.float32)
        assert m.shape[0] == 2 and m.shape[2] == 64
        wave = np.empty((2, 240 * m.shape[1]), dtype=np.float32)
        self._ck(lib.ltx_vocoder_forward(self._h, _ptr(m), m.shape[1], _ptr(wave)))
        return wave

    def vocoder_forward_dev(self, mel, waveform):
        self._ck(lib.ltx_vocoder_forward_dev(self._h, _ptr(mel), mel.shape[1], _ptr(waveform)))

    def audio_decode(self, latent):
        """``decodeAudio``: latent (8, T, 16) f32 -> waveform (2, audio_sample_count(T)) f32 (host arrays)."""
        lat = np.ascontiguousarray(latent, dtype=np.float32)
        assert lat.shape[0] == 8 and lat.shape[2] == 16
        wave = np.empty((2, audio_sample_count(lat.shape[1])), dtype=np.float32)
        self._ck(lib.ltx_audio_decode(self._h, _ptr(lat), lat.shape[1], _ptr(wave)))
        return wave

    def audio_decode_dev(self, latent, waveform):
        self._ck(lib.ltx_audio_decode_dev(self._h, _ptr(latent), latent.shape[1], _ptr(waveform)))

    def op_conv1d(self, x, w, bias, dilation=1, tile=-1, resid=None, f32_act=0, transposed=False, out_f32=None, bf16_act=0, slope=0.1,
                  out_bf16=None):
        L, Cin = x.shape
        Cout, k, _ = w.shape
        self._ck(lib.ltx_op_conv1d(self._h, _ptr(x), L, Cin, _ptr(w), _ptr(bias), Cout, k, dilation, tile, _ptr(resid), f32_act,
                                   int(transposed), _ptr(out_f32), bf16_act, slope, _ptr(out_bf16)))

    def op_conv_transpose1d(self, x, w, bias, stride, padding, tile=-1, out_f32=None, bf16_act=0, slope=0.1, out_bf16=None):
        L, Cin = x.shape
        _, Cout, k = w.shape
        self._ck(lib.ltx_op_conv_transpose1d(self._h, _ptr(x), L, Cin, _ptr(w), _ptr(bias), Cout, k, stride, padding, tile, _ptr(out_f32),
                                             bf16_act, slope, _ptr(out_bf16)))

    def op_conv2d_causal(self, x, w, bias, ksize=3, tile=-1, resid=None, transposed=False, out_f32=None, out_bf16=None):
        H, W, Cin = x.shape
        Cout = w.shape[0]
        self._ck(lib.ltx_op_conv2d_causal(self._h, _ptr(x), H, W, Cin, _ptr(w), _ptr(bias), Cout, ksize, tile, _ptr(resid),
                                          int(transposed), _ptr(out_f32), _ptr(out_bf16)))

    # ---- text-embedding connector ----
    def connector_load(self, path, cfg=None):
        self._ck(lib.ltx_connector_load(self._h, str(path).encode(), C.byref(cfg) if cfg is not None else None))

    def connector_init_synthetic(self, cfg=None, seed=91):
        self._ck(lib.ltx_connector_init_synthetic(self._h, C.byref(cfg) if cfg is not None else None, seed))

    def connector_unload(self):
        self._ck(lib.ltx_connector_unload(self._h))

    def connector_encode(self, hidden_bits, attention_mask, padding_right=False):
        """``encodeFromHiddenStates``: hidden [states,B,T,dim] uint16 (bf16 bits), mask [B,T] int32 -> (context bits
        [B,T,dim] uint16, mask [B,T] int32). HOST arrays."""
        h = np.ascontiguousarray(hidden_bits, dtype=np.uint16)
        m = np.ascontiguousarray(attention_mask, dtype=np.int32)
        _, B, T, D = h.shape
        out = np.empty((B, T, D), dtype=np.uint16)
        om = np.empty((B, T), dtype=np.int32)
        self._ck(lib.ltx_connector_encode(self._h, _ptr(h), _ptr(m), B, T, int(padding_right), _ptr(out), _ptr(om)))
        return out, om

    def connector_encode_dev(self, hidden, attention_mask, context, out_mask=None, padding_right=False, taps=None):
        """Device tensors: hidden [states,B,T,dim] bf16, mask [B,T] int32, context [B,T,dim] bf16. taps = optional
        (norm_concat, fe_out, after_registers) device tensors for parity tests."""
        _, B, T, _ = hidden.shape
        if taps is not None:
            self._ck(lib.ltx_connector_encode_taps_dev(self._h, _ptr(hidden), _ptr(attention_mask), B, T, int(padding_right),
                                                       _ptr(context), _ptr(taps[0]), _ptr(taps[1]), _ptr(taps[2])))
        else:
            self._ck(lib.ltx_connector_encode_dev(self._h, _ptr(hidden), _ptr(attention_mask), B, T, int(padding_right),
                                                  _ptr(context), _ptr(out_mask)))

    def connector_has_audio(self):
        """``ltx_connector_has_audio``: whether the loaded connector has the audio weight set."""
        return bool(lib.ltx_connector_has_audio(self._h))

    def connector_encode_av_dev(self, hidden, attention_mask, video_context, audio_context, out_mask=None, padding_right=False):
        """``ltx_connector_encode_av_dev``: the feature extractor once, then the video and the audio connector. Device tensors; both
        contexts [B,T,dim] bf16."""
        _, B, T, _ = hidden.shape
        self._ck(lib.ltx_connector_encode_av_dev(self._h, _ptr(hidden), _ptr(attention_mask), B, T, int(padding_right), _ptr(video_context),
                                                 _ptr(audio_context), _ptr(out_mask)))

    def connector_encode_av(self, hidden_bits, attention_mask, padding_right=False):
        """``ltx_connector_encode_av``: HOST arrays -> (video context bits, audio context bits, mask)."""
        h = np.ascontiguousarray(hidden_bits, dtype=np.uint16)
        m = np.ascontiguousarray(attention_mask, dtype=np.int32)
        _, B, T, D = h.shape
        out, outa = np.empty((B, T, D), dtype=np.uint16), np.empty((B, T, D), dtype=np.uint16)
        om = np.empty((B, T), dtype=np.int32)
        self._ck(lib.ltx_connector_encode_av(self._h, _ptr(h), _ptr(m), B, T, int(padding_right), _ptr(out), _ptr(outa), _ptr(om)))
        return out, outa, om

    # ---- Gemma-3 text encoder (csrc/gemma.h) ----
    def gemma_load(self, paths, cfg=None):
        """``ltx_gemma_load``: one path or a list of safetensors shards."""
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        self._ck(lib.ltx_gemma_load(self._h, arr, len(paths), C.byref(cfg) if cfg is not None else None))

    def gemma_init_synthetic(self, cfg=None, seed=0):
        self._ck(lib.ltx_gemma_init_synthetic(self._h, C.byref(cfg) if cfg is not None else None, seed))

    def gemma_unload(self):
        self._ck(lib.ltx_gemma_unload(self._h))

    def gemma_memory_info(self):
        """``ltx_gemma_memory_info``: device bytes of the parameters and of the activation workspaces; zeros without a model."""
        w, ws = C.c_long(), C.c_long()
        self._ck(lib.ltx_gemma_memory_info(self._h, C.byref(w), C.byref(ws)))
        return {"weights": w.value, "workspace": ws.value}

    def gemma_encode_dev(self, token_ids, attention_mask, hidden):
        """Device tensors: ids, mask [B,T] int32 -> hidden [layers+1,B,T,hidden] bf16 (the connector's input)."""
        B, T = token_ids.shape
        self._ck(lib.ltx_gemma_encode_dev(self._h, _ptr(token_ids), _ptr(attention_mask), B, T, _ptr(hidden)))

    def gemma_encode(self, token_ids, attention_mask, layers, hidden_size):
        """HOST arrays: ids, mask [B,T] int32 -> hidden bits [layers+1,B,T,hidden] uint16."""
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        m = np.ascontiguousarray(attention_mask, dtype=np.int32)
        B, T = ids.shape
        out = np.empty((layers + 1, B, T, hidden_size), dtype=np.uint16)
        self._ck(lib.ltx_gemma_encode(self._h, _ptr(ids), _ptr(m), B, T, _ptr(out)))
        return out

    def text_encode_dev(self, token_ids, attention_mask, context, out_mask=None):
        """``ltx_text_encode_dev``: the encoder, then the loaded connector. Device tensors; context [B,T,dim] bf16."""
        B, T = token_ids.shape
        self._ck(lib.ltx_text_encode_dev(self._h, _ptr(token_ids), _ptr(attention_mask), B, T, _ptr(context), _ptr(out_mask)))

    def text_encode(self, token_ids, attention_mask, dim):
        """``ltx_text_encode``: HOST arrays ids, mask [B,T] int32 -> (context bits [B,T,dim] uint16, mask [B,T] int32)."""
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        m = np.ascontiguousarray(attention_mask, dtype=np.int32)
        B, T = ids.shape
        out = np.empty((B, T, dim), dtype=np.uint16)
        om = np.empty((B, T), dtype=np.int32)
        self._ck(lib.ltx_text_encode(self._h, _ptr(ids), _ptr(m), B, T, _ptr(out), _ptr(om)))
        return out, om

    def text_av_encode_dev(self, token_ids, attention_mask, video_context, audio_context, out_mask=None):
        """``ltx_text_av_encode_dev``: the encoder, then both connectors. Device tensors; contexts [B,T,dim] bf16."""
        B, T = token_ids.shape
        self._ck(lib.ltx_text_av_encode_dev(self._h, _ptr(token_ids), _ptr(attention_mask), B, T, _ptr(video_context), _ptr(audio_context),
                                            _ptr(out_mask)))

    def text_av_encode(self, token_ids, attention_mask, dim):
        """``ltx_text_av_encode``: HOST arrays ids, mask [B,T] int32 -> (video context bits, audio context bits, mask)."""
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        m = np.ascontiguousarray(attention_mask, dtype=np.int32)
        B, T = ids.shape
        out, outa = np.empty((B, T, dim), dtype=np.uint16), np.empty((B, T, dim), dtype=np.uint16)
        om = np.empty((B, T), dtype=np.int32)
        self._ck(lib.ltx_text_av_encode(self._h, _ptr(ids), _ptr(m), B, T, _ptr(out), _ptr(outa), _ptr(om)))
        return out, outa, om

    def op_attention_causal(self, Q, K, Vt, O, scale, key_start=None, head_dim=256):
        """``ltx_op_attention_causal``: Q / O [B,T,Hq*hd], K [B,T,Hkv*hd], Vt [B,Hkv*hd,ldvt] bf16, key_start [B] int32 or None."""
        B, T, Dq = Q.shape
        self._ck(lib.ltx_op_attention_causal(self._h, _ptr(Q), _ptr(K), _ptr(Vt), Vt.shape[2], _ptr(key_start), B, Dq // head_dim,
                                             K.shape[2] // head_dim, T, head_dim, scale, _ptr(O)))

    def op_attention_causal_ld(self, Q, ldq, q_bstride, K, ldk, k_bstride, Vt, ldvt, vt_bstride, O, ldo, o_bstride, B, Hq, Hkv, T, scale,
                               key_start=None, head_dim=256):
        """``ltx_op_attention_causal_ld``: the same launch with explicit strides in elements. Q / K / Vt / O are bf16 device tensors of
        which only the first element's address is taken, so each may be a view into a longer buffer (not contiguous)."""
        self._ck(lib.ltx_op_attention_causal_ld(self._h, Q.data_ptr(), ldq, q_bstride, K.data_ptr(), ldk, k_bstride, Vt.data_ptr(), ldvt,
                                                vt_bstride, _ptr(key_start), B, Hq, Hkv, T, head_dim, scale, O.data_ptr(), ldo, o_bstride))

    def op_gemma_norm(self, r, w, h=None, x=None, w2=None, n=None, eps=1e-6):
        """``ltx_op_gemma_norm``: r / x / h / n [rows,D] bf16, w / w2 [D] f32."""
        rows, D = r.shape
        self._ck(lib.ltx_op_gemma_norm(self._h, _ptr(r), _ptr(w), _ptr(x), _ptr(w2), rows, D, eps, _ptr(h), _ptr(n)))

    def op_gemma_qknorm_rope(self, qk, wq, wk, q_heads, k_heads, cos, sin, T, eps=1e-6):
        """``ltx_op_gemma_qknorm_rope``: qk [rows,(q_heads+k_heads)*256] bf16, in place."""
        rows, ld = qk.shape
        self._ck(lib.ltx_op_gemma_qknorm_rope(self._h, _ptr(qk), ld, _ptr(wq), _ptr(wk), q_heads, k_heads, _ptr(cos), _ptr(sin), T, rows, eps))

    def op_gemma_rope_tables(self, T, base, cos, sin):
        self._ck(lib.ltx_op_gemma_rope_tables(self._h, T, base, _ptr(cos), _ptr(sin)))

    def op_geglu(self, gu, out):
        rows, I2 = gu.shape
        self._ck(lib.ltx_op_geglu(self._h, _ptr(gu), rows, I2 // 2, _ptr(out)))

    def op_gemma_embed(self, ids, table, out):
        vocab, D = table.shape
        self._ck(lib.ltx_op_gemma_embed(self._h, _ptr(ids), _ptr(table), ids.numel(), D, vocab, _ptr(out)))

    # ---- Gemma-3 token generation on a KV cache (csrc/gemma.h, second half) ----
    def lm_begin(self, capacity):
        self._ck(lib.ltx_lm_begin(self._h, capacity))

    def lm_end(self):
        """``ltx_lm_end``: the bytes released."""
        n = C.c_long()
        self._ck(lib.ltx_lm_end(self._h, C.byref(n)))
        return n.value

    def lm_memory_info(self):
        c, w = C.c_long(), C.c_long()
        self._ck(lib.ltx_lm_memory_info(self._h, C.byref(c), C.byref(w)))
        return {"cache": c.value, "workspace": w.value}

    def lm_prefill_dev(self, ids, logits=None):
        """Device tensors: ids [T] int32, logits [vocab] f32 or None."""
        self._ck(lib.ltx_lm_prefill_dev(self._h, _ptr(ids), ids.numel(), _ptr(logits)))

    def lm_prefill(self, ids, vocab=None):
        """HOST ids -> the last position's logits [vocab] f32 (None without ``vocab``)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        out = np.empty(vocab, np.float32) if vocab else None
        self._ck(lib.ltx_lm_prefill(self._h, _ptr(ids), ids.size, _ptr(out)))
        return out

    def lm_step_dev(self, token, logits=None):
        self._ck(lib.ltx_lm_step_dev(self._h, _ptr(token), _ptr(logits)))

    def lm_step(self, token, vocab=None):
        out = np.empty(vocab, np.float32) if vocab else None
        self._ck(lib.ltx_lm_step(self._h, int(token), _ptr(out)))
        return out

    def lm_last_state(self, hidden_size):
        """model.norm of the newest position: bf16 bits [hidden_size] uint16."""
        out = np.empty(hidden_size, np.uint16)
        self._ck(lib.ltx_lm_last_state(self._h, _ptr(out)))
        return out

    def lm_cache_k(self, layer, rows, width):
        """Rows 0 .. rows-1 of a layer's K cache: bf16 bits [rows, width] uint16 (width = num_key_value_heads * 256)."""
        out = np.empty((rows, width), np.uint16)
        self._ck(lib.ltx_lm_cache_k(self._h, layer, rows, _ptr(out)))
        return out

    def lm_cache_vt(self, layer, cols, width):
        """Columns 0 .. cols-1 of a layer's V^T cache: bf16 bits [width, cols] uint16 (width = num_key_value_heads * 256; cols up to the
        padded width roundup(capacity, 64))."""
        out = np.empty((width, cols), np.uint16)
        self._ck(lib.ltx_lm_cache_vt(self._h, layer, cols, _ptr(out)))
        return out

    def lm_generate(self, ids, params=None):
        """``ltx_lm_generate``: HOST ids [T] -> the generated ids (int32 array), stop id excluded."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if params is None:
            params = lm_params()
        out = np.zeros(max(params.max_new_tokens, 1), np.int32)
        n = C.c_int()
        self._ck(lib.ltx_lm_generate(self._h, _ptr(ids), ids.size, C.byref(params), _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def op_gemv_bf16(self, x, W, N, K, epilogue=0, out_bf16=None, out_stride=1, out_f32=None, ldw=None, M=1):
        """``ltx_op_gemv_bf16``: x [K] and W [rows, ldw] bf16 device tensors; epilogue 0 bf16 store, 1 f32 store, 2 GeGLU."""
        self._ck(lib.ltx_op_gemv_bf16(self._h, _dptr(x), _dptr(W), (W.shape[-1] if W is not None else 0) if ldw is None else ldw, M, N, K, epilogue, _dptr(out_bf16), out_stride,
                                      _dptr(out_f32)))

    def op_attention_decode(self, q, K, Vt, O, Hq, Hkv, n_keys, scale, ldk=None, ldvt=None):
        """``ltx_op_attention_decode``: q / O [Hq*256], K [cap, ldk], Vt [Hkv*256, ldvt] bf16 device tensors."""
        self._ck(lib.ltx_op_attention_decode(self._h, _dptr(q), _dptr(K), (K.shape[-1] if K is not None else 0) if ldk is None else ldk, _dptr(Vt),
                                             (Vt.shape[-1] if Vt is not None else 0) if ldvt is None else ldvt, Hq, Hkv, n_keys, scale, _dptr(O)))

    def op_lm_pick(self, logits, out, hist=None, n_gen=0, context=64, penalty=1.0, vocab=None):
        """``ltx_op_lm_pick``: logits [vocab] f32 (penalised in place), hist int32 [>= n_gen + 1] or None, out int32 [1]."""
        self._ck(lib.ltx_op_lm_pick(self._h, _dptr(logits), logits.numel() if vocab is None else vocab, _dptr(hist), n_gen, context, penalty, _dptr(out)))

    # ---- helper passes (include/ltxhip.h, "Test seams of the helper passes"): device tensors, sizes given explicitly, so that a
    # tensor may be longer than the pass's extent (guard elements behind it) or a view into a longer one (vae_prepare's chan_stride) ----
    def op_mean_var(self, x, n_per_batch, B, stats):
        self._ck(lib.ltx_op_mean_var(self._h, _dptr(x), n_per_batch, B, _dptr(stats)))

    def op_guidance_rescale(self, cfg, stats_cfg, stats_cond, phi, n_per_batch, B):
        self._ck(lib.ltx_op_guidance_rescale(self._h, _dptr(cfg), _dptr(stats_cfg), _dptr(stats_cond), phi, n_per_batch, B))

    def op_adain(self, x, stats_x, stats_ref, factor, n_per_chan, BC):
        self._ck(lib.ltx_op_adain(self._h, _dptr(x), _dptr(stats_x), _dptr(stats_ref), factor, n_per_chan, BC))

    def op_groupnorm_stats(self, x, P, C, G, eps, stats):
        self._ck(lib.ltx_op_groupnorm_stats(self._h, _dptr(x), P, C, G, eps, _dptr(stats)))

    def op_groupnorm_apply(self, x, stats, w, b, P, C, G, resid=None, act_silu=False, out_f32=None, out_bf16=None):
        self._ck(lib.ltx_op_groupnorm_apply(self._h, _dptr(x), _dptr(stats), _dptr(w), _dptr(b), _dptr(resid), int(act_silu), _dptr(out_f32),
                                            _dptr(out_bf16), P, C, G))

    def op_pixelnorm_silu(self, x, out, P, C, scale=None, shift=None):
        self._ck(lib.ltx_op_pixelnorm_silu(self._h, _dptr(x), _dptr(scale), _dptr(shift), _dptr(out), P, C))

    def op_vae_prepare(self, latent, chan_stride, mean, std, out, C, P, noise=None, noise_scale=0.0):
        self._ck(lib.ltx_op_vae_prepare(self._h, _dptr(latent), chan_stride, _dptr(noise), noise_scale, _dptr(mean), _dptr(std), _dptr(out), C, P))

    def op_upscaler_finish(self, x, mean, std, out, P, C):
        self._ck(lib.ltx_op_upscaler_finish(self._h, _dptr(x), _dptr(mean), _dptr(std), _dptr(out), P, C))

    def op_blend_frames(self, r, nx, n_frames, frame_elems):
        self._ck(lib.ltx_op_blend_frames(self._h, _dptr(r), _dptr(nx), n_frames, frame_elems))

    def op_patchify_bf16(self, latent, tokens, B, C, T):
        self._ck(lib.ltx_op_patchify_bf16(self._h, _dptr(latent), _dptr(tokens), B, C, T))

    def op_unpatchify_f32(self, tokens, latent, B, C, T):
        self._ck(lib.ltx_op_unpatchify_f32(self._h, _dptr(tokens), _dptr(latent), B, C, T))

    def op_euler_step(self, latent, velocity, sigma, sigma_next, n, skip_hw=0, frames=1):
        self._ck(lib.ltx_op_euler_step(self._h, _dptr(latent), _dptr(velocity), sigma, sigma_next, n, skip_hw, frames))

    def op_set_frame0(self, latent, cond, C, F, HW, noise=None, scale=0.0, sigma2=0.0):
        self._ck(lib.ltx_op_set_frame0(self._h, _dptr(latent), _dptr(cond), _dptr(noise), scale, sigma2, C, F, HW))

    def op_make_mod(self, tables, ada, mod, B, L, J, D):
        self._ck(lib.ltx_op_make_mod(self._h, _dptr(tables), _dptr(ada), _dptr(mod), B, L, J, D))

    def op_fe_stats(self, hidden, mask, states, B, T, D, partials, stats, padding_right=False, eps=1e-6):
        """``ltx_op_fe_stats``: partials holds at least ``fe_stats_partials_floats(states, B, T, D)`` f32."""
        self._ck(lib.ltx_op_fe_stats(self._h, _dptr(hidden), _dptr(mask), states, B, T, D, int(padding_right), eps, _dptr(partials), _dptr(stats)))

    def op_fe_norm_concat(self, hidden, mask, stats, states, B, T, D, out, padding_right=False, eps=1e-6):
        self._ck(lib.ltx_op_fe_norm_concat(self._h, _dptr(hidden), _dptr(mask), _dptr(stats), states, B, T, D, int(padding_right), eps, _dptr(out)))

    # ---- the remaining helper passes (include/ltxhip.h, "Test seams of the remaining helper passes") ----
    def op_cfg_combine(self, uncond, cond, scale, out, n):
        self._ck(lib.ltx_op_cfg_combine(self._h, _dptr(uncond), _dptr(cond), scale, _dptr(out), n))

    def op_lincomb(self, a, b, ca, cb, out, n):
        self._ck(lib.ltx_op_lincomb(self._h, _dptr(a), _dptr(b), ca, cb, _dptr(out), n))

    def op_axpby(self, a, b, ca, cb, out, n):
        self._ck(lib.ltx_op_axpby(self._h, _dptr(a), _dptr(b), ca, cb, _dptr(out), n))

    def op_ge(self, a, b, g, out, n):
        self._ck(lib.ltx_op_ge(self._h, _dptr(a), _dptr(b), g, _dptr(out), n))

    def op_scale_inplace(self, x, s, n):
        self._ck(lib.ltx_op_scale_inplace(self._h, _dptr(x), s, n))

    def op_clip01(self, x, n):
        self._ck(lib.ltx_op_clip01(self._h, _dptr(x), n))

    def op_mask_to_bias(self, mask, bias, n):
        self._ck(lib.ltx_op_mask_to_bias(self._h, _dptr(mask), _dptr(bias), n))

    def op_cast_f32_bf16(self, x, out, n):
        self._ck(lib.ltx_op_cast_f32_bf16(self._h, _dptr(x), _dptr(out), n))

    def op_cast_bf16_f32(self, x, out, n):
        self._ck(lib.ltx_op_cast_bf16_f32(self._h, _dptr(x), _dptr(out), n))

    def op_timestep_embedding(self, ts, mult, out, n, dim):
        self._ck(lib.ltx_op_timestep_embedding(self._h, _dptr(ts), mult, _dptr(out), n, dim))

    def op_vae_make_mods_batch(self, jobs):
        """``ltx_op_vae_make_mods_batch``: jobs = [(table, te or None, out, rows, C), ...] of device tensors, one launch."""
        arr = (_lib.VaeModsJob * max(len(jobs), 1))()
        for j, (table, te, out, rows, Cc) in zip(arr, jobs):
            j.table, j.te, j.out, j.rows, j.C = _dptr(table), _dptr(te), _dptr(out), rows, Cc
        self._ck(lib.ltx_op_vae_make_mods_batch(self._h, arr, len(jobs)))

    def op_sp_vt_interleave(self, gathered, vt, N, D, Tn, ld):
        self._ck(lib.ltx_op_sp_vt_interleave(self._h, _dptr(gathered), _dptr(vt), N, D, Tn, ld))

    def op_register_plan(self, mask, B, T, src):
        self._ck(lib.ltx_op_register_plan(self._h, _dptr(mask), B, T, _dptr(src)))

    def op_register_gather(self, enc, registers, src, B, T, D, R, x):
        self._ck(lib.ltx_op_register_gather(self._h, _dptr(enc), _dptr(registers), _dptr(src), B, T, D, R, _dptr(x)))

    def op_enc_patchify(self, pixels, out, T, H, W):
        self._ck(lib.ltx_op_enc_patchify(self._h, _dptr(pixels), _dptr(out), T, H, W))

    def op_enc_s2d_residual(self, conv, Cc, x, Cx, out, Cout, T, H, W, ft, fh, fw):
        self._ck(lib.ltx_op_enc_s2d_residual(self._h, _dptr(conv), Cc, _dptr(x), Cx, _dptr(out), Cout, T, H, W, ft, fh, fw))

    def op_enc_finish(self, z, ldz, out, C, P, mean=None, std=None):
        self._ck(lib.ltx_op_enc_finish(self._h, _dptr(z), ldz, _dptr(mean), _dptr(std), _dptr(out), C, P))

    def op_i2v_rowmap(self, row_map, B, T, first, G):
        self._ck(lib.ltx_op_i2v_rowmap(self._h, _dptr(row_map), B, T, first, G))

    def op_i2v_timesteps(self, ts, B, G, sigma):
        self._ck(lib.ltx_op_i2v_timesteps(self._h, _dptr(ts), B, G, sigma))

    def op_fill_const_i32(self, p, n, v):
        self._ck(lib.ltx_op_fill_const_i32(self._h, _dptr(p), n, v))

    def op_gemma_mask_scan(self, mask, B, T, key_start, status):
        self._ck(lib.ltx_op_gemma_mask_scan(self._h, _dptr(mask), B, T, _dptr(key_start), _dptr(status)))

    def op_audio_pn_pad(self, x, H, W, C, mode, out):
        self._ck(lib.ltx_op_audio_pn_pad(self._h, _dptr(x), H, W, C, mode, _dptr(out)))

    def op_audio_upsample_pad(self, x, H, W, C, out):
        self._ck(lib.ltx_op_audio_upsample_pad(self._h, _dptr(x), H, W, C, _dptr(out)))

    def op_audio_denorm_pad(self, latent, mean, std, Cl, T, Wl, Cpad, out):
        self._ck(lib.ltx_op_audio_denorm_pad(self._h, _dptr(latent), _dptr(mean), _dptr(std), Cl, T, Wl, Cpad, _dptr(out)))

    def op_audio_mel_pack(self, mel, T, M, out):
        self._ck(lib.ltx_op_audio_mel_pack(self._h, _dptr(mel), T, M, _dptr(out)))

    def op_audio_mean3_act(self, a, b, c, rows, C, slope, out, ldb):
        self._ck(lib.ltx_op_audio_mean3_act(self._h, _dptr(a), _dptr(b), _dptr(c), rows, C, slope, _dptr(out), ldb))

    def upscaler_load(self, path):
        self._ck(lib.ltx_upscaler_load(self._h, str(path).encode()))

    def upscaler_unload(self):
        self._ck(lib.ltx_upscaler_unload(self._h))

    def upscale_latent(self, latent):
        """``upsampleLatents``: [1,128,F,H,W] f32 -> [1,128,F,2H,2W] f32 (needs the VAE's statistics loaded)."""
        lat = np.ascontiguousarray(latent, dtype=np.float32)
        _, Cc, F, H, W = lat.shape
        out = np.empty((1, Cc, F, 2 * H, 2 * W), dtype=np.float32)
        self._ck(lib.ltx_upscale_latent(self._h, _ptr(lat), F, H, W, _ptr(out)))
        return out

    def upscale_latent_dev(self, latent, out):
        """``ltx_upscale_latent_dev``: device tensors, latent [1,128,F,H,W] f32 -> out [1,128,F,2H,2W] f32; asynchronous."""
        _, _, F, H, W = latent.shape
        self._ck(lib.ltx_upscale_latent_dev(self._h, _ptr(latent), F, H, W, _ptr(out)))

    def adain_filter_latent(self, latent, reference, factor=1.0):
        lat = np.ascontiguousarray(latent, dtype=np.float32).copy()
        ref = np.ascontiguousarray(reference, dtype=np.float32)
        Cc = lat.shape[1]
        self._ck(lib.ltx_adain_filter_latent(self._h, _ptr(lat), lat[0, 0].size, _ptr(ref), ref[0, 0].size, Cc, factor))
        return lat

    def generate_two_stage(self, noise1, noise2, context_bf16, mask, width, height, num_frames, num_steps=8, vae_tile=0,
                           decode=True, on_progress=None):
        """Host-level mirror of ``generateVideoTwoStage`` (LTXPipeline.swift:2420-2741) for the distilled T2V case:
        stage 1 at W/2 x H/2, latent upscale x2, AdaIN against the stage-1 latent, re-noise with the explicit
        ``noise2`` at sigma 0.909375, 3-step stage-2 refinement (never CFG), decode. Noise tensors are explicit
        inputs (the reference draws them from MLX's global RNG)."""
        validate_generation_config(width, height, num_frames, num_steps, 1.0, two_stage=True)
        F1, H1, W1 = latent_shape(width // 2, height // 2, num_frames)
        F2, H2, W2 = latent_shape(width, height, num_frames)
        sig1 = sigmas(True, num_steps, F1 * H1 * W1)
        lat = np.ascontiguousarray(noise1, dtype=np.float32) * sig1[0]
        lat = self.denoise(lat, sig1, context_bf16, mask, F1, H1, W1, on_progress=on_progress)
        stage1 = lat
        lat = self.upscale_latent(lat)
        lat = self.adain_filter_latent(lat, stage1)
        s2 = stage2_sigmas()
        lat = (np.float32(s2[0]) * np.asarray(noise2, np.float32) + np.float32(1.0 - s2[0]) * lat).astype(np.float32)
        lat = self.denoise(lat, s2, context_bf16, mask, F2, H2, W2, on_progress=on_progress)
        if not decode:
            return lat
        return self.vae_decode(lat, tile=vae_tile)

    # ---- denoise loop ----
    @staticmethod
    def _options(cfg_scale=1.0, guidance_rescale=0.0, stg_scale=0.0, stg_blocks=(29,), ge_gamma=0.0, cond_latent=None,
                 image_cond_noise_scale=0.0, cond_noise=None, shard=SHARD_NONE, step_stats=None):
        """cond_latent / cond_noise (image-to-video): numpy arrays for the host entry point, torch tensors for the device one.
        step_stats: a C-contiguous float32 numpy array [n_steps, 4] that receives (velocity mean, velocity std, latent mean, latent std)
        per step - the reference's --profile diagnostics (LTXPipeline.swift:945-951)."""
        arr = (C.c_int * max(1, len(stg_blocks)))(*stg_blocks)
        if isinstance(cond_latent, np.ndarray):
            cond_latent = np.ascontiguousarray(cond_latent, dtype=np.float32)
        if isinstance(cond_noise, np.ndarray):
            cond_noise = np.ascontiguousarray(cond_noise, dtype=np.float32)
        if step_stats is not None:
            assert isinstance(step_stats, np.ndarray) and step_stats.dtype == np.float32 and step_stats.flags["C_CONTIGUOUS"] and step_stats.shape[-1] == 4
        o = DenoiseOptions(C.sizeof(DenoiseOptions), cfg_scale, guidance_rescale, stg_scale, C.cast(arr, C.POINTER(C.c_int)), len(stg_blocks), ge_gamma,
                           _ptr(cond_latent), image_cond_noise_scale, _ptr(cond_noise), int(shard), _ptr(step_stats))
        o._keep = (arr, cond_latent, cond_noise, step_stats)
        return o

    def denoise(self, latent, sigmas_, context_bf16, mask, F, H, W, on_progress=None, **opts):
        """Host-pointer denoise loop. latent [1,C,F,H,W] f32 (scaled by sigmas[0]); returns the final latent."""
        lat = np.ascontiguousarray(latent, dtype=np.float32).copy()
        sg = np.ascontiguousarray(sigmas_, dtype=np.float32)
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        c = np.ascontiguousarray(context_bf16)
        o = self._options(**opts)
        self._ck(lib.ltx_denoise(self._h, _ptr(lat), F, H, W, sg.ctypes.data_as(C.POINTER(C.c_float)), len(sg), _ptr(c), _ptr(m),
                                 c.shape[1], C.byref(o), cb, None))
        return lat

    def denoise_dev(self, latent, sigmas_, context, mask, F, H, W, ctx_version=1, mask_all_ones=False, on_progress=None, **opts):
        sg = np.ascontiguousarray(sigmas_, dtype=np.float32)
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        o = self._options(**opts)
        self._ck(lib.ltx_denoise_dev(self._h, _ptr(latent), F, H, W, sg.ctypes.data_as(C.POINTER(C.c_float)), len(sg), _ptr(context),
                                     _ptr(mask), int(mask_all_ones), context.shape[1], ctx_version, C.byref(o), cb, None))

    # ---- live kernel timing ----
    def prof_enable(self, on=True):
        self._ck(lib.ltx_prof_enable(self._h, int(on)))

    def prof_collect(self, kind, reset=False):
        ms, n, w = C.c_double(), C.c_long(), C.c_double()
        self._ck(lib.ltx_prof_collect(self._h, kind, C.byref(ms), C.byref(n), C.byref(w), int(reset)))
        return {"ms": ms.value, "launches": n.value, "work": w.value}

    # ---- kernel-level hooks (device tensors) ----
    def op_gemm(self, A, B, bias=None, act=0, tile_cfg=-1, out_f32=None, out_bf16=None):
        M, K = A.shape
        N = B.shape[0]
        self._ck(lib.ltx_op_gemm_bf16(self._h, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(bias), M, N, K, act, tile_cfg,
                                      _ptr(out_f32), out_f32.stride(0) if out_f32 is not None else 0,
                                      _ptr(out_bf16), out_bf16.stride(0) if out_bf16 is not None else 0))

    def op_gemm_q8(self, A, codes, scales, biases, bias, out, split_k=1, via_scratch=False, tile_cfg=30):
        """out[M][N] f32 = A[M][K] bf16 . dequant(codes [N][K] u8, scales / biases [N][K/64] bf16)^T + bias"""
        M, K = A.shape
        N = codes.shape[0]
        self._ck(lib.ltx_op_gemm_q8(self._h, _ptr(A), A.stride(0), _ptr(codes), _ptr(scales), _ptr(biases), _ptr(bias), M, N, K, split_k,
                                    int(via_scratch), tile_cfg, _ptr(out), out.stride(0)))

    def op_value_projection_t(self, X, W, bias, vt):
        tokens, K = X.shape
        self._ck(lib.ltx_op_value_projection_t(self._h, _ptr(X), X.stride(0), tokens, _ptr(W), _ptr(bias), W.shape[0], K, _ptr(vt), vt.stride(0)))

    def op_qkv_projection(self, X, Wqk, bqk, Wv, bv, qk_out, vt_out, rows=None, rows_per_batch=None, fused=True):
        """qk_out[:rows, :2 D] bf16 = X[:rows, :K] . Wqk^T + bqk; V^T per batch element b of rows_per_batch rows in the attention op's
        layout: row b * D + d of vt_out (any shape with rows of ldvt = vt_out.stride(-2) elements) holds (X . Wv^T + bv)[:, d] of that
        element's rows. Wqk [2 D][K] and Wv [D][K] dense; X, qk_out and vt_out may have wider rows than they use. fused: one launch of
        192 x 384 tiles (an error on a shape it does not take), else the two-launch path. Same bits either way."""
        D, K = Wv.shape
        rows = X.shape[0] if rows is None else rows
        self._ck(lib.ltx_op_qkv_projection(self._h, _ptr(X), X.stride(0), rows, rows if rows_per_batch is None else rows_per_batch, _ptr(Wqk),
                                           _ptr(bqk), _ptr(Wv), _ptr(bv), D, K, _ptr(qk_out), qk_out.stride(0), _ptr(vt_out), vt_out.stride(-2),
                                           int(fused)))

    def op_gemm_gated_residual(self, A, B, bias, gate, gate_scalar, x, mirror=None):
        M, K = A.shape
        N = B.shape[0]
        self._ck(lib.ltx_op_gemm_bf16_gated_residual(self._h, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(bias), _ptr(gate),
                                                     gate_scalar, M, N, K, _ptr(x), x.stride(0), _ptr(mirror),
                                                     mirror.stride(0) if mirror is not None else 0))

    def op_gemm_gated_residual_norm(self, A, B, bias, gate, gate_scalar, x, scale, shift, xn, eps=1e-6, fused=True):
        M, K = A.shape
        N = B.shape[0]
        self._ck(lib.ltx_op_gemm_bf16_gated_residual_norm(self._h, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(bias), _ptr(gate),
                                                          gate_scalar, M, N, K, _ptr(x), x.stride(0), _ptr(scale), _ptr(shift), eps,
                                                          _ptr(xn), xn.stride(0), int(fused)))

    def op_gemv(self, a, W, bias, out, in_act=0):
        M, K = a.shape
        N = W.shape[0]
        self._ck(lib.ltx_op_gemv_f32(self._h, _ptr(a), a.stride(0), _ptr(W), W.stride(0), _ptr(bias), _ptr(out), out.stride(0), M, N, K, in_act))

    def op_attention(self, Q, K, Vt, bias, H, O, scale=None):
        B, Tq, _ = Q.shape
        Tk = K.shape[1]
        ldvt = Vt.shape[2]
        if scale is None:
            scale = 1.0 / (128.0 ** 0.5)
        self._ck(lib.ltx_op_attention(self._h, _ptr(Q), _ptr(K), _ptr(Vt), ldvt, _ptr(bias), B, H, Tq, Tk, scale, _ptr(O)))

    @staticmethod
    def attention_key_splits(B, H, Tq, Tk):
        """Key ranges the attention launcher divides a launch of this shape into (1 = no split)."""
        return lib.ltx_attention_key_splits(B, H, Tq, Tk)

    def op_attention_hd(self, Q, K, Vt, bias, H, O, head_dim, scale=None):
        """``ltx_op_attention_hd``: Q / K / O [B][T][H*head_dim], Vt [B][H*head_dim][ldvt]; scale <= 0: Q is prescaled."""
        B, Tq, _ = Q.shape
        Tk = K.shape[1]
        if scale is None:
            scale = 1.0 / (float(head_dim) ** 0.5)
        self._ck(lib.ltx_op_attention_hd(self._h, _ptr(Q), _ptr(K), _ptr(Vt), Vt.shape[2], _ptr(bias), B, H, Tq, Tk, head_dim, scale, _ptr(O)))

    @staticmethod
    def attention_hd_workgroup_queries(B, H, Tq, head_dim=64):
        """Queries per workgroup the launcher picks for a head-dim-64 launch of this shape (256, 128 or 64)."""
        return lib.ltx_attention_hd_workgroup_queries(B, H, Tq, head_dim)

    def op_qknorm_rope_hd(self, x, w, cos, sin, T, out, head_dim, out_scale=1.0, eps=1e-6):
        rows, D = out.shape
        self._ck(lib.ltx_op_qknorm_rope_hd(self._h, _ptr(x), x.stride(0), _ptr(w), _ptr(cos), _ptr(sin), T, rows, D, head_dim, out_scale, eps,
                                           _ptr(out)))

    # ---- LTXAttention at head dim 64: the audio / cross-modal attention modules of the dual block ----
    def attn_module_init_synthetic(self, index, query_dim, context_dim=0, heads=32, seed=4242):
        self._ck(lib.ltx_attn_module_init_synthetic(self._h, index, query_dim, context_dim, heads, seed))

    def attn_module_load(self, index, path, key_prefix, heads=32):
        self._ck(lib.ltx_attn_module_load(self._h, index, str(path).encode(), key_prefix.encode(), heads))

    def attn_module_unload(self, index):
        self._ck(lib.ltx_attn_module_unload(self._h, index))

    def attn_module_export_param(self, index, name):
        """One resident parameter of module ``index`` as a flat f32 numpy array ("to_q.weight", ..., "k_norm.weight")."""
        n = lib.ltx_attn_module_export_param(self._h, index, name.encode(), None, 0)
        if n < 0:
            raise LTXError(-n, lib.ltx_last_error(self._h).decode(errors="replace"))
        out = np.empty(n, dtype=np.float32)
        n2 = lib.ltx_attn_module_export_param(self._h, index, name.encode(), out.ctypes.data, n)
        if n2 < 0:
            raise LTXError(-n2, lib.ltx_last_error(self._h).decode(errors="replace"))
        return out

    def attn_module_forward_dev(self, index, x, out, context=None, q_tables=None, k_tables=None, key_bias=None):
        """``ltx_attn_module_forward_dev``: x [B][Tq][Dq] f32, context [B][Tk][Dc] f32 or bf16 (None: self-attention), q_tables /
        k_tables = (cos, sin) device tensors [rows][heads*32] f32 or None, key_bias [B][Tk] f32 or None, out [B][Tq][Dq] f32."""
        B, Tq, _ = x.shape
        Tk = Tq if context is None else context.shape[1]
        qc, qs = q_tables if q_tables is not None else (None, None)
        kc, ks = k_tables if k_tables is not None else (None, None)
        self._ck(lib.ltx_attn_module_forward_dev(self._h, index, _ptr(x), _ptr(context), int(context is not None and context.element_size() == 2),
                                                 B, Tq, Tk, _ptr(qc), _ptr(qs), 0 if qc is None else qc.shape[0], _ptr(kc), _ptr(ks),
                                                 0 if kc is None else kc.shape[0], _ptr(key_bias), _ptr(out)))

    # ---- LTX2TransformerBlock x L: the dual video + audio transformer blocks ----
    def dual_blocks_init_synthetic(self, cfg, seed=4242):
        self._ck(lib.ltx_dual_blocks_init_synthetic(self._h, C.byref(cfg), seed))

    def dual_blocks_load(self, path, cfg, first_block=0, num_blocks=None):
        self._ck(lib.ltx_dual_blocks_load(self._h, str(path).encode(), C.byref(cfg), first_block, cfg.num_layers if num_blocks is None else num_blocks))

    def dual_blocks_unload(self):
        self._ck(lib.ltx_dual_blocks_unload(self._h))

    def dual_blocks_export_param(self, name):
        """One resident parameter of the stack as a flat f32 numpy array ("transformer_blocks.0.attn1.to_q.weight", ...)."""
        n = lib.ltx_dual_blocks_export_param(self._h, name.encode(), None, 0)
        if n < 0:
            raise LTXError(-n, lib.ltx_last_error(self._h).decode(errors="replace"))
        out = np.empty(n, dtype=np.float32)
        n2 = lib.ltx_dual_blocks_export_param(self._h, name.encode(), out.ctypes.data, n)
        if n2 < 0:
            raise LTXError(-n2, lib.ltx_last_error(self._h).decode(errors="replace"))
        return out

    def dual_blocks_forward_dev(self, x_video, x_audio, context_video, context_audio, temb_video, temb_audio, cross_video_ss, cross_audio_ss,
                                F, H, W, key_bias_video=None, key_bias_audio=None, phase_mask=0, struct_size=None, T_a=None, n_groups=1,
                                video_row_map=None):
        """``ltx_dual_blocks_forward_dev``: device tensors; x_video [B][F*H*W][Dv] and x_audio [B][T_a][Da] f32 are updated in place,
        the contexts [B][S][.] are bf16, temb_* [B][6][D], cross_*_ss [B][5][D] f32, key biases [B][S] f32 or None. With timestep groups
        (``n_groups`` > 1, ``video_row_map`` [B*F*H*W] int32) temb_video / cross_video_ss have B * n_groups rows."""
        a = DualForwardArgs()
        a.struct_size = C.sizeof(DualForwardArgs) if struct_size is None else struct_size
        a.B, a.F, a.H, a.W = x_video.shape[0], F, H, W
        a.T_a = x_audio.shape[1] if T_a is None else T_a
        a.S = context_video.shape[1]
        a.x_video, a.x_audio = _ptr(x_video), _ptr(x_audio)
        a.context_video, a.context_audio = _ptr(context_video), _ptr(context_audio)
        a.key_bias_video, a.key_bias_audio = _ptr(key_bias_video), _ptr(key_bias_audio)
        a.temb_video, a.temb_audio = _ptr(temb_video), _ptr(temb_audio)
        a.cross_video_ss, a.cross_audio_ss = _ptr(cross_video_ss), _ptr(cross_audio_ss)
        a.phase_mask = phase_mask
        a.n_groups, a.video_row_map = n_groups, _ptr(video_row_map)
        self._ck(lib.ltx_dual_blocks_forward_dev(self._h, C.byref(a)))

    # ---- LTX2Transformer: the dual video + audio model ----
    def dual_model_init_synthetic(self, cfg, seed=4242):
        self._ck(lib.ltx_dual_model_init_synthetic(self._h, C.byref(cfg), seed))

    def dual_model_load(self, path, cfg, quant_bits=16):
        """``ltx_dual_model_load``; ``quant_bits`` 8 or 4 then quantises the loaded model (``dual_model_quantize``), as the reference
        quantises ``LTX2Transformer`` right after building it (LTXPipeline.swift:487-492). 16: bf16."""
        self._ck(lib.ltx_dual_model_load(self._h, str(path).encode(), C.byref(cfg)))
        if quant_bits != 16:
            self.dual_model_quantize(quant_bits)

    def dual_model_quantize(self, bits, group_size=64):
        """``ltx_dual_model_quantize``: ``quantize(model: ltx2, groupSize: 64, bits:)`` (LTXPipeline.swift:487-492)."""
        self._ck(lib.ltx_dual_model_quantize(self._h, bits, group_size))

    def dual_model_memory_info(self):
        """``ltx_dual_model_memory_info`` as ``dit_memory_info``'s dict (LTXPipeline.swift:3176-3187); all zero without a model."""
        v = [C.c_long() for _ in range(4)]
        self._ck(lib.ltx_dual_model_memory_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("bf16_weights", "quantised_weights", "scratch", "other"), (x.value for x in v)))

    def dual_model_unload(self):
        self._ck(lib.ltx_dual_model_unload(self._h))

    def dual_model_export_param(self, name):
        """One resident parameter of the model as a flat f32 numpy array ("adaln_single.linear.weight", "transformer_blocks.0. ...")."""
        n = lib.ltx_dual_model_export_param(self._h, name.encode(), None, 0)
        if n < 0:
            raise LTXError(-n, lib.ltx_last_error(self._h).decode(errors="replace"))
        out = np.empty(n, dtype=np.float32)
        n2 = lib.ltx_dual_model_export_param(self._h, name.encode(), out.ctypes.data, n)
        if n2 < 0:
            raise LTXError(-n2, lib.ltx_last_error(self._h).decode(errors="replace"))
        return out

    def dual_model_forward_groups_dev(self, video_latent, audio_latent, video_context, audio_context, video_timesteps, audio_timesteps,
                                      video_velocity, audio_velocity, F, H, W, n_groups, video_row_map, **kw):
        """``ltx_dual_model_forward_groups_dev``: ``dual_model_forward_dev`` with timestep groups on the video stream: video_timesteps
        [B][n_groups] f32, video_row_map [B*F*H*W] int32 (b * n_groups + group) or None with one group; see ``timestep_groups``."""
        self.dual_model_forward_dev(video_latent, audio_latent, video_context, audio_context, video_timesteps, audio_timesteps, video_velocity,
                                    audio_velocity, F, H, W, _groups=(int(n_groups), video_row_map), **kw)

    def dual_model_forward_dev(self, video_latent, audio_latent, video_context, audio_context, video_timesteps, audio_timesteps,
                               video_velocity, audio_velocity, F, H, W, video_mask=None, audio_mask=None, ungrouped=False, struct_size=None,
                               T_a=None, text_cache=0, S=None, _groups=None):
        """``ltx_dual_model_forward_dev``: device tensors; latents [B][T][C] and contexts [B][S][caption_channels] bf16, timesteps [B] f32
        (sigma), masks [B][S] int32 or None; the velocities [B][F*H*W][out_channels] / [B][T_a][audio_out_channels] f32 are written.
        ``text_cache`` non-zero reads the text side from ``dual_model_prepare_text``: the contexts and masks may be None (give ``S``)."""
        a = DualModelForwardArgs()
        a.struct_size = C.sizeof(DualModelForwardArgs) if struct_size is None else struct_size
        a.B, a.F, a.H, a.W = video_latent.shape[0], F, H, W
        a.T_a = audio_latent.shape[1] if T_a is None else T_a
        a.S = video_context.shape[1] if S is None else S
        a.text_cache = int(text_cache)
        a.video_latent, a.audio_latent = _ptr(video_latent), _ptr(audio_latent)
        a.video_context, a.audio_context = _ptr(video_context), _ptr(audio_context)
        a.video_timesteps, a.audio_timesteps = _ptr(video_timesteps), _ptr(audio_timesteps)
        a.video_mask, a.audio_mask = _ptr(video_mask), _ptr(audio_mask)
        a.video_velocity, a.audio_velocity = _ptr(video_velocity), _ptr(audio_velocity)
        a.ungrouped = int(ungrouped)
        if _groups is not None:
            self._ck(lib.ltx_dual_model_forward_groups_dev(self._h, C.byref(a), _groups[0], _ptr(_groups[1])))
            return
        self._ck(lib.ltx_dual_model_forward_dev(self._h, C.byref(a)))

    def dual_model_embed_dev(self, video_timesteps, audio_timesteps, temb_v, temb_a, cross_v, cross_a, embts_v, embts_a, ungrouped=False, B=None):
        """``ltx_dual_model_embed_dev``: the timestep path alone into caller tensors (f32, device)."""
        self._ck(lib.ltx_dual_model_embed_dev(self._h, _ptr(video_timesteps), _ptr(audio_timesteps),
                                              video_timesteps.shape[0] if B is None else B, int(ungrouped), _ptr(temb_v), _ptr(temb_a),
                                              _ptr(cross_v), _ptr(cross_a), _ptr(embts_v), _ptr(embts_a)))

    def dual_model_prepare_text(self, video_context, audio_context, video_mask=None, audio_mask=None, B=None, S=None):
        """``ltx_dual_model_prepare_text_dev``: the text side of the forwards of one prompt, once (contexts [B][S][caption_channels] bf16,
        masks [B][S] int32 or None; device tensors)."""
        self._ck(lib.ltx_dual_model_prepare_text_dev(self._h, _ptr(video_context), _ptr(audio_context), _ptr(video_mask), _ptr(audio_mask),
                                                     video_context.shape[0] if B is None else B, video_context.shape[1] if S is None else S))

    def dual_model_text_cache_info(self):
        """``ltx_dual_model_text_cache_info`` as a dict(B=, S=, bytes=, builds=)."""
        B, S, nb, builds = C.c_int(), C.c_int(), C.c_long(), C.c_long()
        self._ck(lib.ltx_dual_model_text_cache_info(self._h, C.byref(B), C.byref(S), C.byref(nb), C.byref(builds)))
        return {"B": B.value, "S": S.value, "bytes": nb.value, "builds": builds.value}

    @staticmethod
    def _dual_denoise_args(video_latent, audio_latent, sg, video_context, audio_context, mask, F, H, W, T_a, S, cfg_scale, guidance_rescale,
                           text_cache, stats, struct_size, cond_latent=None, image_cond_noise_scale=0.0, cond_noise=None):
        a = DualDenoiseArgs()
        a.struct_size = C.sizeof(DualDenoiseArgs) if struct_size is None else struct_size
        a.F, a.H, a.W, a.T_a, a.S = F, H, W, T_a, S
        a.video_latent, a.audio_latent = _ptr(video_latent), _ptr(audio_latent)
        a.sigmas, a.n_sigmas = sg.ctypes.data_as(C.POINTER(C.c_float)), len(sg)
        a.video_context, a.audio_context, a.mask = _ptr(video_context), _ptr(audio_context), _ptr(mask)
        a.cfg_scale, a.guidance_rescale, a.text_cache = cfg_scale, guidance_rescale, int(text_cache)
        a.step_stats = None if stats is None else stats.ctypes.data
        a.cond_latent, a.image_cond_noise_scale, a.cond_noise = _ptr(cond_latent), image_cond_noise_scale, _ptr(cond_noise)
        return a

    def dual_denoise_dev(self, video_latent, audio_latent, sigmas_, video_context, F, H, W, audio_context=None, mask=None, cfg_scale=1.0,
                         guidance_rescale=0.0, text_cache=1, step_stats=False, on_progress=None, T_a=None, S=None, struct_size=None,
                         cond_latent=None, image_cond_noise_scale=0.0, cond_noise=None):
        """``ltx_dual_denoise_dev``: the joint loop on device tensors, in place. video_latent [1][C][F][H][W] f32 and audio_latent
        [1][8][T_a][16] f32, scaled by sigmas[0]; contexts [nb][S][caption_channels] bf16, nb = 2 ([negative, positive]) iff cfg_scale > 1;
        mask [nb][S] int32 or None. Image-to-video: cond_latent [1][C][1][H][W] f32 and, for re-noising, image_cond_noise_scale > 0 with
        cond_noise [steps][C][1][H][W] f32. Returns the step statistics [steps][8] when ``step_stats``, else None."""
        sg = np.ascontiguousarray(sigmas_, dtype=np.float32)
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        stats = np.zeros((max(len(sg) - 1, 0), 8), np.float32) if step_stats else None
        a = self._dual_denoise_args(video_latent, audio_latent, sg, video_context, audio_context, mask, F, H, W,
                                    audio_latent.shape[2] if T_a is None else T_a, video_context.shape[1] if S is None else S, cfg_scale,
                                    guidance_rescale, text_cache, stats, struct_size, cond_latent, image_cond_noise_scale, cond_noise)
        self._ck(lib.ltx_dual_denoise_dev(self._h, C.byref(a), cb, None))
        return stats

    def dual_denoise(self, video_latent, audio_latent, sigmas_, video_context_bf16, F, H, W, audio_context_bf16=None, mask=None, cfg_scale=1.0,
                     guidance_rescale=0.0, text_cache=1, step_stats=False, on_progress=None, cond_latent=None, image_cond_noise_scale=0.0,
                     cond_noise=None):
        """``ltx_dual_denoise``: the same with host arrays (contexts as bf16 bit patterns, uint16; cond_latent / cond_noise f32). Returns
        (video_latent, audio_latent) or, with ``step_stats``, (video_latent, audio_latent, stats)."""
        cl = None if cond_latent is None else np.ascontiguousarray(cond_latent, dtype=np.float32)
        cn = None if cond_noise is None else np.ascontiguousarray(cond_noise, dtype=np.float32)
        v = np.ascontiguousarray(video_latent, dtype=np.float32).copy()
        au = np.ascontiguousarray(audio_latent, dtype=np.float32).copy()
        sg = np.ascontiguousarray(sigmas_, dtype=np.float32)
        cv = np.ascontiguousarray(video_context_bf16)
        ca = None if audio_context_bf16 is None else np.ascontiguousarray(audio_context_bf16)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        stats = np.zeros((max(len(sg) - 1, 0), 8), np.float32) if step_stats else None
        a = self._dual_denoise_args(v, au, sg, cv, ca, mk, F, H, W, au.shape[2], cv.shape[1], cfg_scale, guidance_rescale, text_cache, stats, None,
                                    cl, image_cond_noise_scale, cn)
        self._ck(lib.ltx_dual_denoise(self._h, C.byref(a), cb, None))
        return (v, au, stats) if step_stats else (v, au)

    def op_dual_step(self, video=None, audio=None, sigma=1.0, sigma_next=0.0):
        """``ltx_op_dual_step``: each job is None or a dict(latent=, v_cond=, tokens= tensors, v_uncond=None, v_out=None, cfg_scale=1.0,
        form=0, copies=1, n= latent.numel(), n_keep=0, keep_src=None, keep_noise=None, keep_scale=0.0)."""
        def job(j):
            if j is None:
                return None
            o = DualStepJob()
            o.n_keep, o.keep_scale = j.get("n_keep", 0), j.get("keep_scale", 0.0)
            for k in ("latent", "v_cond", "v_uncond", "tokens", "v_out", "keep_src", "keep_noise"):
                t = j.get(k)
                setattr(o, k, None if t is None else t.data_ptr())
            o.cfg_scale, o.form, o.copies = j.get("cfg_scale", 1.0), j.get("form", 0), j.get("copies", 1)
            o.n = j["n"] if "n" in j else j["latent"].numel()
            return C.byref(o)
        self._ck(lib.ltx_op_dual_step(self._h, job(video), job(audio), sigma, sigma_next))

    def op_dual_restage(self, video=None, audio=None):
        """``ltx_op_dual_restage``: each job is None or a dict of device tensors and scalars. video: x= [C][T] f32, latent= [T][C] f32 (out),
        tokens= [T][C] bf16 (out), noise= [C][T] or None, noise_scale=, and either stats= / stats_ref= ([C][2]) or ref= [C][T_ref] (the
        stage-1 output; the statistics are then computed), stats_out= [4*C] or None, cond= [C][HW] or None, cond_noise=, cond_scale=,
        cond_sigma2=. audio: latent= [T][C] f32 (in / out), tokens=, noise= [T][C] or None, noise_scale=. ``renoise`` defaults to whether
        noise is given; C, T, T_ref and HW default to the tensors' shapes."""
        def job(j, is_video):
            if j is None:
                return None
            o = DualRestageJob()
            for k in ("x", "latent", "tokens", "noise", "stats", "stats_ref", "ref", "stats_out", "cond", "cond_noise"):
                t = j.get(k)
                setattr(o, k, None if t is None else t.data_ptr())
            lat = j.get("latent")
            if is_video and j.get("x") is not None:
                o.C, o.T = j["x"].shape[0], j["x"][0].numel()
            elif lat is not None:
                o.C, o.T = lat.shape[-1], lat.numel() // lat.shape[-1]
            o.C, o.T = j.get("C", o.C), j.get("T", o.T)
            o.noise_scale = j.get("noise_scale", 0.0)
            o.renoise = int(j.get("renoise", j.get("noise") is not None))
            o.T_ref = j.get("T_ref", j["ref"][0].numel() if j.get("ref") is not None else 0)
            o.HW = j.get("HW", j["cond"][0].numel() if j.get("cond") is not None else 0)
            o.cond_scale, o.cond_sigma2 = j.get("cond_scale", 0.0), j.get("cond_sigma2", 0.0)
            return C.byref(o)
        self._ck(lib.ltx_op_dual_restage(self._h, job(video, True), job(audio, False)))

    @staticmethod
    def _dual_two_stage_args(video_latent_in, video_latent_out, audio_latent, sg1, sg2, video_noise2, audio_noise2, video_context, audio_context,
                             mask, F, H, W, T_a, S, stage1_out, cond_latent1, cond_latent2, image_cond_noise_scale, cond_noise1, cond_noise2,
                             struct_size=None):
        a = DualTwoStageArgs()
        a.struct_size = C.sizeof(DualTwoStageArgs) if struct_size is None else struct_size
        a.F, a.H, a.W, a.T_a, a.S = F, H, W, T_a, S
        a.video_latent_in, a.video_latent_out, a.audio_latent = _ptr(video_latent_in), _ptr(video_latent_out), _ptr(audio_latent)
        a.sigmas1, a.n_sigmas1 = sg1.ctypes.data_as(C.POINTER(C.c_float)), len(sg1)
        if sg2 is not None:
            a.sigmas2, a.n_sigmas2 = sg2.ctypes.data_as(C.POINTER(C.c_float)), len(sg2)
        a.video_noise2, a.audio_noise2 = _ptr(video_noise2), _ptr(audio_noise2)
        a.video_context, a.audio_context, a.mask = _ptr(video_context), _ptr(audio_context), _ptr(mask)
        a.stage1_out = _ptr(stage1_out)
        a.cond_latent1, a.cond_latent2, a.image_cond_noise_scale = _ptr(cond_latent1), _ptr(cond_latent2), image_cond_noise_scale
        a.cond_noise1, a.cond_noise2 = _ptr(cond_noise1), _ptr(cond_noise2)
        return a

    def dual_two_stage_dev(self, video_latent_in, video_latent_out, audio_latent, sigmas1, video_noise2, audio_noise2, video_context, F, H, W,
                           sigmas2=None, audio_context=None, mask=None, stage1_out=None, cond_latent1=None, cond_latent2=None,
                           image_cond_noise_scale=0.0, cond_noise1=None, cond_noise2=None, on_progress=None, T_a=None, S=None, struct_size=None):
        """``ltx_dual_two_stage_dev``: both stages of the two-stage video + audio path on device tensors. video_latent_in [1][128][F][H][W] f32
        scaled by sigmas1[0] (not written), video_latent_out [1][128][F][2H][2W] f32, audio_latent [1][8][T_a][16] f32 in place;
        video_noise2 as video_latent_out, audio_noise2 [T_a][128] (the packed shape); sigmas2 None = ``stage2_sigmas()``. Image-to-video:
        cond_latent1 [1][128][1][H][W] and cond_latent2 [1][128][1][2H][2W], with cond_noise1 / cond_noise2 [steps][128][1][h][w] for
        re-noising. F, H, W are the STAGE-1 latent dims."""
        sg1 = np.ascontiguousarray(sigmas1, dtype=np.float32)
        sg2 = None if sigmas2 is None else np.ascontiguousarray(sigmas2, dtype=np.float32)
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        a = self._dual_two_stage_args(video_latent_in, video_latent_out, audio_latent, sg1, sg2, video_noise2, audio_noise2, video_context,
                                      audio_context, mask, F, H, W, audio_latent.shape[2] if T_a is None else T_a,
                                      video_context.shape[1] if S is None else S, stage1_out, cond_latent1, cond_latent2, image_cond_noise_scale,
                                      cond_noise1, cond_noise2, struct_size)
        self._ck(lib.ltx_dual_two_stage_dev(self._h, C.byref(a), cb, None))

    def dual_two_stage(self, video_latent, audio_latent, sigmas1, video_noise2, audio_noise2, video_context_bf16, sigmas2=None,
                       audio_context_bf16=None, mask=None, stage1_out=False, cond_latent1=None, cond_latent2=None, image_cond_noise_scale=0.0,
                       cond_noise1=None, cond_noise2=None, on_progress=None):
        """``ltx_dual_two_stage``: the same with host arrays (contexts as bf16 bit patterns, uint16). video_latent is the stage-1 latent
        [1][128][F][H][W]. Returns (video_latent [1][128][F][2H][2W], audio_latent) or, with ``stage1_out``, (video, audio, stage-1 video)."""
        f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)  # noqa: E731
        v = f32(video_latent)
        _, Cc, F, H, W = v.shape
        out = np.zeros((1, Cc, F, 2 * H, 2 * W), np.float32)
        au = f32(audio_latent).copy()
        s1 = np.zeros_like(v) if stage1_out else None
        sg1 = f32(sigmas1)
        sg2 = f32(sigmas2)
        cv = np.ascontiguousarray(video_context_bf16)
        ca = None if audio_context_bf16 is None else np.ascontiguousarray(audio_context_bf16)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        keep = [f32(video_noise2), f32(audio_noise2), f32(cond_latent1), f32(cond_latent2), f32(cond_noise1), f32(cond_noise2)]
        a = self._dual_two_stage_args(v, out, au, sg1, sg2, keep[0], keep[1], cv, ca, mk, F, H, W, au.shape[2], cv.shape[1], s1, keep[2], keep[3],
                                      image_cond_noise_scale, keep[4], keep[5])
        self._ck(lib.ltx_dual_two_stage(self._h, C.byref(a), cb, None))
        return (out, au, s1) if stage1_out else (out, au)

    def op_mlx_normal_group(self, jobs, n_jobs=None):
        """``ltx_op_mlx_normal_group``: each job is a dict(key= two uint32, dst= a device tensor or None, n= dst.numel(), scale=1.0,
        raw_bits=False). One launch for up to 64 jobs."""
        arr = (NoiseJob * max(len(jobs), 1))()
        for o, j in zip(arr, jobs):
            o.key[0], o.key[1] = int(j["key"][0]), int(j["key"][1])
            dst = j.get("dst")
            o.dst = None if dst is None else dst.data_ptr()
            o.n = j["n"] if "n" in j else dst.numel()
            o.scale, o.raw_bits = j.get("scale", 1.0), int(bool(j.get("raw_bits", False)))
        self._ck(lib.ltx_op_mlx_normal_group(self._h, arr, len(jobs) if n_jobs is None else n_jobs))

    def mlx_random_normal_dev(self, seed, out, draw_index=0, scale=1.0, n=None):
        """``ltx_mlx_random_normal_dev``: ``mlx_random_normal`` into the device f32 tensor ``out``, times scale."""
        self._ck(lib.ltx_mlx_random_normal_dev(self._h, int(seed), int(draw_index), _ptr(out), out.numel() if n is None else n, scale))

    def dual_generate_dev(self, args, on_progress=None):
        """``ltx_dual_generate_dev`` on a struct from ``dual_generate_args`` (device tensors)."""
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        self._ck(lib.ltx_dual_generate_dev(self._h, C.byref(args) if args is not None else None, cb, None))

    def dual_generate(self, args, on_progress=None):
        """``ltx_dual_generate`` on a struct from ``dual_generate_args`` (host arrays; contexts as bf16 bit patterns)."""
        cb = PROGRESS_CB(on_progress if on_progress else (lambda s, t, sig, u: None))
        self._ck(lib.ltx_dual_generate(self._h, C.byref(args) if args is not None else None, cb, None))

    def op_gemv_group(self, jobs, M=None, n_jobs=None):
        """``ltx_op_gemv_group``: each job is a dict(a= [M][K] f32, W= [N][K] bf16, out= a 2-D f32 view whose row stride is ldo, bias=
        tensor or None, in_act=0); N / K default to W's shape and may be given (N=0 skips the job; a / W / out may then be None)."""
        arr = (GemvJob * max(1, len(jobs)))()
        for o, j in zip(arr, jobs):
            a, W, out = j.get("a"), j.get("W"), j.get("out")
            o.a, o.lda = (a.data_ptr(), j.get("lda", a.stride(0))) if a is not None else (None, j.get("lda", 0))
            o.W, o.ldw = (W.data_ptr(), j.get("ldw", W.stride(0))) if W is not None else (None, j.get("ldw", 0))
            o.out, o.ldo = (out.data_ptr(), out.stride(0)) if out is not None else (None, 0)
            o.bias = _ptr(j.get("bias"))
            o.N = j["N"] if "N" in j else W.shape[0]
            o.K = j["K"] if "K" in j else W.shape[1]
            o.in_act = j.get("in_act", 0)
        if M is None:
            M = jobs[0]["a"].shape[0]
        self._ck(lib.ltx_op_gemv_group(self._h, arr, len(jobs) if n_jobs is None else n_jobs, M))

    def op_gemv_group_q(self, jobs, bits, M=None, n_jobs=None):
        """``ltx_op_gemv_group_q`` (the timestep path of a quantised LTX2Transformer, LTX2Transformer.swift:272-312): each job is a
        dict(a= [M][K] f32, codes= [N][K * bits / 8] uint8, scales=, biases= [N][K / 64] bf16, out= a 2-D f32 view whose row stride is ldo,
        bias= tensor or None, in_act=0); N defaults to the codes' rows and K to scales' columns x 64, and both may be given."""
        arr = (GemvJobQ * max(1, len(jobs)))()
        for o, j in zip(arr, jobs):
            a, codes, scales, out = j.get("a"), j.get("codes"), j.get("scales"), j.get("out")
            o.a, o.lda = (a.data_ptr(), j.get("lda", a.stride(0))) if a is not None else (None, j.get("lda", 0))
            o.codes, o.scales, o.biases, o.bias = _ptr(codes), _ptr(scales), _ptr(j.get("biases")), _ptr(j.get("bias"))
            o.out, o.ldo = (out.data_ptr(), out.stride(0)) if out is not None else (None, 0)
            o.N = j["N"] if "N" in j else codes.shape[0]
            o.K = j["K"] if "K" in j else scales.shape[1] * 64
            o.in_act = j.get("in_act", 0)
        if M is None:
            M = jobs[0]["a"].shape[0]
        self._ck(lib.ltx_op_gemv_group_q(self._h, arr, len(jobs) if n_jobs is None else n_jobs, M, bits))

    def op_norm_mod2(self, video=None, audio=None, eps=1e-6):
        """``ltx_op_norm_mod2``: each job is None or a dict(x=, out0=, out1= 2-D tensors whose row strides are ldx / ldo, rows=, D=,
        scale0=, shift0=, scale1=, shift1= (tensors or None), mod_bstride=0, rows_per_batch=rows, row_map=None ([rows] int32))."""
        def job(j):
            if j is None:
                return None
            o = NormMod2Job()
            o.x, o.ldx = j["x"].data_ptr(), j["x"].stride(0)
            for k in ("scale0", "shift0", "scale1", "shift1"):
                setattr(o, k, _ptr(j.get(k)))
            o.mod_bstride = j.get("mod_bstride", 0)
            o.rows_per_batch = j.get("rows_per_batch", max(1, j["rows"]))
            o.out0, o.out1, o.ldo = j["out0"].data_ptr(), j["out1"].data_ptr(), j["out0"].stride(0)
            o.rows, o.D = j["rows"], j["D"]
            o.row_map = _ptr(j.get("row_map"))
            return C.byref(o)
        self._ck(lib.ltx_op_norm_mod2(self._h, job(video), job(audio), eps))

    def op_norm_mod(self, x, scale, shift, out, norm_kind=0, eps=1e-6, round_norm_bf16=False):
        rows, D = x.shape
        self._ck(lib.ltx_op_norm_mod(self._h, _ptr(x), _ptr(scale), _ptr(shift), rows, D, norm_kind, eps, int(round_norm_bf16), _ptr(out)))

    def op_qknorm_rope(self, x, w, cos, sin, T, out, eps=1e-6):
        rows, D = out.shape
        self._ck(lib.ltx_op_qknorm_rope(self._h, _ptr(x), x.stride(0), _ptr(w), _ptr(cos), _ptr(sin), T, rows, D, eps, _ptr(out)))

    def op_norm_mod_ex(self, x, scale, shift, out, rows, D, mod_bstride=0, rows_per_batch=None, row_map=None, norm_kind=0, eps=1e-6,
                       round_norm_bf16=False):
        """``ltx_op_norm_mod_ex``: x / out are 2-D tensors whose row strides are ldx / ldo (``rows`` x ``D`` of them are used)."""
        self._ck(lib.ltx_op_norm_mod_ex(self._h, x.data_ptr(), x.stride(0), _ptr(scale), _ptr(shift), mod_bstride,
                                        rows if rows_per_batch is None else rows_per_batch, _ptr(row_map), rows, D, norm_kind, eps,
                                        int(round_norm_bf16), out.data_ptr(), out.stride(0)))

    def op_qknorm_rope_pair(self, x0, w0, out0, x1, w1, out1, cos, sin, T, rows, D, eps=1e-6, out_scale0=1.0):
        """``ltx_op_qknorm_rope_pair``: x0 / x1 are views of f32 or bf16 rows with one row stride (x1 None: one job)."""
        assert x1 is None or (x1.stride(0) == x0.stride(0) and out1.stride(0) == out0.stride(0) and x1.dtype == x0.dtype)
        vp = lambda t: None if t is None else t.data_ptr()  # strided views of wider buffers
        self._ck(lib.ltx_op_qknorm_rope_pair(self._h, vp(x0), _ptr(w0), vp(out0), vp(x1), _ptr(w1), vp(out1), x0.stride(0),
                                             out0.stride(0), _ptr(cos), _ptr(sin), T, rows, D, eps, out_scale0,
                                             int(x0.element_size() == 2)))

    def op_fill_normal_bf16(self, t, seed, mean=0.0, std=1.0):
        self._ck(lib.ltx_op_fill_normal_bf16(self._h, _ptr(t), t.numel(), seed, mean, std))

    def op_fill_normal_f32(self, t, seed, mean=0.0, std=1.0):
        self._ck(lib.ltx_op_fill_normal_f32(self._h, _ptr(t), t.numel(), seed, mean, std))


# ---------------------------------------------------------------------------------------------------------------
# bf16 helpers for host arrays (bit patterns as uint16)
# ---------------------------------------------------------------------------------------------------------------
def f32_to_bf16_bits(x):
    """Round-to-nearest-even f32 -> bf16 bit patterns (uint16), numpy."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return r.reshape(x.shape)


def bf16_bits_to_f32(b):
    b = np.ascontiguousarray(b, dtype=np.uint16)
    return (b.astype(np.uint32) << 16).view(np.float32).reshape(b.shape)
