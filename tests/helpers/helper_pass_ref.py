"""Plain numpy float64 restatements of the helper passes of csrc/elementwise.h (guidance, scheduler, VAE decoder and encoder, latent
upscaler, connector, timestep embedding, casts) and of the row passes of csrc/audio.h, written from the formulas in those headers and
the reference seams they cite, one array expression per formula. Inputs are taken as they are (f32 or bf16 VALUES held in any float
array) and widened to float64; nothing here rounds, except `bf16*` (the output format of the bf16 passes), `set_frame0_f32` (whose
contract is a float32 replay) and `timestep_embedding_f32` (the float32 replay that measures that pass's bound). Scalars that a kernel
receives as f32 must be passed as the f32 value (np.float32(0.4), not 0.4): `f32()` does that."""
import numpy as np

F64 = np.float64
U = 2.0 ** -24          # unit roundoff of f32: one correctly rounded operation has relative error <= U
EPS_STD = float(np.float32(1e-8))


def f32(v):
    """The float64 value of v rounded to f32: what a kernel sees of a scalar argument."""
    return float(np.float32(v))


def gamma(k):
    """Higham's gamma_k: bound of the relative error accumulated by k roundings, (1 + U)^k - 1 <= k U / (1 - k U)."""
    return k * U / (1.0 - k * U)


# ---- bf16 as an output format ----
def bf16(x):
    """float64 -> nearest bf16 value (8 significant bits, ties to even) in ONE rounding, returned as float64."""
    m, e = np.frexp(np.asarray(x, F64))          # x = m * 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 256.0), e - 8)   # np.rint rounds half to even


def bf16_ulp(x):
    """Spacing of bf16 values at |x| (0 at x == 0)."""
    x = np.asarray(x, F64)
    _, e = np.frexp(x)
    return np.where(x == 0, 0.0, np.ldexp(1.0, e - 8))


def bf16_bits(x):
    """Bit patterns (uint16) of values that ARE bf16 values."""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(x32.astype(F64), np.asarray(x, F64)), "not f32 values"
    u = x32.view(np.uint32)
    assert not (u & 0xFFFF).any(), "not bf16 values"
    return (u >> 16).astype(np.uint16)


def bf16_rne_bits(x):
    """f32 values -> bf16 bit patterns by the definition on the bits (round to nearest, ties to even, of the upper 16 bits), which also
    covers what `bf16` does not: subnormal results, overflow to infinity, the infinities, the sign of zero. NaN is not defined here."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(F64)


# ---- DiT / scheduler ----
def make_mod(tables, ada):
    """mod[b][l][j][d] = table[l][j][d] + ada[b][j][d]"""
    return np.asarray(tables, F64)[None, :, :, :] + np.asarray(ada, F64)[:, None, :, :]


def patchify(latent):
    """[B][C][T] -> [B][T][C]"""
    return np.asarray(latent, F64).transpose(0, 2, 1)


def unpatchify(tokens):
    """[B][T][C] -> [B][C][T]"""
    return np.asarray(tokens, F64).transpose(0, 2, 1)


def euler_step(x, v, sigma, sigma_next, skip_hw=0, frames=1):
    """den = x - s*v; x' = s_next > 0 ? den + s_next*(x - den)/s : den. skip_hw > 0: x is [C][frames][skip_hw] flattened and frame 0 of
    every channel keeps its value. Returns (x', kept) with kept the boolean index of the untouched elements."""
    x, v = np.asarray(x, F64), np.asarray(v, F64)
    s, sn = f32(sigma), f32(sigma_next)
    den = x - s * v
    out = den + sn * (x - den) / s if sn > 0 else den
    kept = np.zeros(x.shape, bool)
    if skip_hw > 0:
        kept = kept.reshape(-1, frames, skip_hw)
        kept[:, 0, :] = True
        kept = kept.reshape(x.shape)
    return np.where(kept, x, out), kept


def set_frame0_f32(latent, cond, noise, scale, sigma2):
    """latent [C][F][HW], cond / noise [C][HW]: frame 0 = cond, or cond + (scale * noise) * sigma2 as three separately rounded FLOAT32
    operations (the contract is bit equality with the reference's array ops). Frames >= 1 are returned as they came."""
    out = np.array(latent, dtype=np.float32, copy=True)
    c = np.asarray(cond, np.float32)
    if noise is not None:
        a = np.float32(scale) * np.asarray(noise, np.float32)
        b = a * np.float32(sigma2)
        c = c + b
    out[:, 0, :] = c
    return out


# ---- guidance ----
def mean_var(x):
    """Population mean and variance over the last axis."""
    x = np.asarray(x, F64)
    m = x.mean(axis=-1)
    return m, ((x - m[..., None]) ** 2).mean(axis=-1)


def guidance_rescale(cfg, var_cfg, var_cond, phi):
    """cfg [B][n]: phi*cfg*(std_cond/std_cfg) + (1 - phi)*cfg with std = sqrt(var + 1e-8)"""
    cfg, p = np.asarray(cfg, F64), f32(phi)
    ratio = np.sqrt(np.asarray(var_cond, F64) + EPS_STD) / np.sqrt(np.asarray(var_cfg, F64) + EPS_STD)
    return p * (cfg * ratio[:, None]) + f32(1.0 - p) * cfg


def adain(x, mean_x, var_x, mean_ref, var_ref, factor):
    """x [BC][n]: y = (x - mu)/(sd + 1e-8)*sd_ref + mu_ref; factor >= 1 ? y : factor*y + (1 - factor)*x"""
    x, f = np.asarray(x, F64), f32(factor)
    col = lambda a: np.asarray(a, F64)[:, None]
    y = (x - col(mean_x)) / (np.sqrt(col(var_x)) + EPS_STD) * np.sqrt(col(var_ref)) + col(mean_ref)
    return y if f >= 1.0 else f * y + f32(1.0 - f) * x


# ---- VAE ----
def vae_prepare(latent, noise, noise_scale, mean, std):
    """latent / noise [C][P] -> [P][C]: v = noise ? noise*s + (1 - s)*latent : latent; v*std[c] + mean[c]"""
    v = np.asarray(latent, F64)
    if noise is not None:
        s = f32(noise_scale)
        v = np.asarray(noise, F64) * s + f32(1.0 - s) * v
    return (v * np.asarray(std, F64)[:, None] + np.asarray(mean, F64)[:, None]).T


def blend_frames(r, nx, n_frames):
    """r, nx [n_frames][elems]: r*(1 - i/n) + nx*(i/n) for frame i"""
    w = (np.arange(n_frames, dtype=F64) / n_frames)[:, None]
    return np.asarray(r, F64) * (1.0 - w) + np.asarray(nx, F64) * w


def silu(y):
    return y / (1.0 + np.exp(-y))


def pixelnorm_silu(x, scale=None, shift=None):
    """x [P][C]: SiLU(x / sqrt(mean_c(x^2) + 1e-8) * scale + shift); scale holds the + 1 already; None: scale 1, shift 0"""
    x = np.asarray(x, F64)
    y = x / np.sqrt((x * x).mean(axis=1, keepdims=True) + EPS_STD)
    if scale is not None:
        y = y * np.asarray(scale, F64)[None, :] + np.asarray(shift, F64)[None, :]
    return silu(y)


# ---- latent upscaler ----
def groupnorm_stats(x, G, eps):
    """x [P][C] -> (mean [G], rstd [G], var [G]) over all positions x the C/G adjacent channels of a group; rstd = 1/sqrt(var + eps)"""
    x = np.asarray(x, F64)
    P, C = x.shape
    m, v = mean_var(x.reshape(P, G, C // G).transpose(1, 0, 2).reshape(G, -1))
    return m, 1.0 / np.sqrt(v + f32(eps)), v


def groupnorm_apply(x, mean, rstd, w, b, resid=None, act_silu=False):
    """out = (x - mean_g)*rstd_g*w[c] + b[c] (+ resid), SiLU when act_silu. Returns (out, t, y, pre): t the product before b, y = t + b,
    pre the value SiLU is applied to - the magnitudes an error bound is counted in."""
    x = np.asarray(x, F64)
    C, G = x.shape[1], len(mean)
    g = np.arange(C) // (C // G)
    t = (x - np.asarray(mean, F64)[g][None, :]) * np.asarray(rstd, F64)[g][None, :] * np.asarray(w, F64)[None, :]
    y = t + np.asarray(b, F64)[None, :]
    pre = y + np.asarray(resid, F64) if resid is not None else y
    return (silu(pre) if act_silu else pre), t, y, pre


def upscaler_finish(x, mean, std):
    """x [P][C] -> [C][P]: (x - mean[c]) / std[c]"""
    return ((np.asarray(x, F64) - np.asarray(mean, F64)[None, :]) / np.asarray(std, F64)[None, :]).T


# ---- connector ----
def fe_valid(mask, padding_right):
    """mask [B][T] -> valid [B][T]: the reference rebuilds the mask from the row's length n (its count of non-zero entries) and the
    padding side: the first n tokens (right padding) or the last n (left padding)."""
    mask = np.asarray(mask)
    B, T = mask.shape
    n = (mask != 0).sum(axis=1)[:, None]
    t = np.arange(T)[None, :]
    return (t < n) if padding_right else (t >= T - n)


def fe_stats(hidden, mask, padding_right, eps):
    """hidden [S][B][T][D] -> (mean, min, max), each [S][B], over the valid tokens: mean = sum / (n*D + eps)"""
    h = np.asarray(hidden, F64)
    S, B, T, D = h.shape
    valid = fe_valid(mask, padding_right)
    n = valid.sum(axis=1)
    v4 = valid[None, :, :, None]
    mean = np.where(v4, h, 0.0).sum(axis=(2, 3)) / (n[None, :] * D + f32(eps))
    mn = np.where(v4, h, np.inf).min(axis=(2, 3))
    mx = np.where(v4, h, -np.inf).max(axis=(2, 3))
    return mean, mn, mx


def register_plan(mask):
    """mask [B][T] -> src [B][T] int32. Row by row: the valid token indices in order, then the padded ones, is the order tokens are
    laid out in; position p keeps its entry of that order where the REVERSED mask is set and is a learnable register (-1) elsewhere."""
    mask = np.asarray(mask)
    src = np.empty(mask.shape, np.int32)
    idx = np.arange(mask.shape[1])
    for b, valid in enumerate(mask != 0):
        order = np.concatenate([idx[valid], idx[~valid]])
        src[b] = np.where(valid[::-1], order, -1)
    return src


def register_gather(enc, registers, src):
    """enc [B][T][D], registers [R][D], src [B][T] -> x [B][T][D]: src >= 0 ? enc[b][src] : registers[p % R]"""
    enc, registers, src = np.asarray(enc, F64), np.asarray(registers, F64), np.asarray(src)
    T, R = src.shape[1], registers.shape[0]
    taken = np.take_along_axis(enc, np.maximum(src, 0)[:, :, None], axis=1)
    return np.where((src >= 0)[:, :, None], taken, np.tile(registers, (-(-T // R), 1))[None, :T, :])


def fe_norm_concat(hidden, mask, mean, range_eps, padding_right):
    """out[b][t][d*S + l] = valid ? 8*(x - mean[l][b]) / range_eps[l][b] : 0   -> [B][T][D*S] (before the rounding to bf16)"""
    h = np.asarray(hidden, F64)
    S, B, T, D = h.shape
    valid = fe_valid(mask, padding_right)
    v = 8.0 * (h - np.asarray(mean, F64)[:, :, None, None]) / np.asarray(range_eps, F64)[:, :, None, None]
    v = np.where(valid[None, :, :, None], v, 0.0)
    return v.transpose(1, 2, 3, 0).reshape(B, T, D * S)


# ---- guidance combines and small elementwise passes ----
def cfg_combine(uncond, cond, scale):
    """cond + (scale - 1) * (cond - uncond); scale - 1 is formed once in f32 (LatentUtils.swift:131-141)"""
    c = np.asarray(cond, F64)
    return c + float(np.float32(scale) - np.float32(1.0)) * (c - np.asarray(uncond, F64))


def lincomb(a, b, ca, cb):
    return f32(ca) * np.asarray(a, F64) + f32(cb) * np.asarray(b, F64)


def axpby(a, b, ca, cb):
    """cb * a + ca * (a - b): STG is v + s * (v - v_perturbed) at cb = 1 (LTXPipeline.swift:920)"""
    a = np.asarray(a, F64)
    return f32(cb) * a + f32(ca) * (a - np.asarray(b, F64))


def ge(a, b, g):
    """g * (a - b) + b (LTXPipeline.swift:924-927)"""
    b = np.asarray(b, F64)
    return f32(g) * (np.asarray(a, F64) - b) + b


def scale(x, s):
    return np.asarray(x, F64) * f32(s)


def clip01(x):
    """(x + 1) / 2 clipped to [0, 1] (VideoDecoder.swift:501-505)"""
    return np.clip((np.asarray(x, F64) + 1.0) / 2.0, 0.0, 1.0)


def mask_to_bias(mask):
    """1 -> 0, 0 -> -10000 (LTXTransformer.swift:141-156); the zero is +0"""
    return (1.0 - np.asarray(mask, F64)) * -10000.0 + 0.0


def vae_make_mods(table, te=None):
    """table, te [rows][C]: table + te + (1 on odd rows: the scale rows hold scale + 1) (VideoDecoder.swift:93-113)"""
    t = np.asarray(table, F64)
    out = t + (np.asarray(te, F64) if te is not None else 0.0)
    out[1::2] += 1.0
    return out


def timestep_frequencies(dim, dtype=F64):
    """f_k = exp(-ln(10000) * k / half), k < half = dim / 2, each operation in `dtype`"""
    half = dim // 2
    k = np.arange(half).astype(dtype)
    return np.exp(-np.log(dtype(10000.0)) * (k / dtype(half)))


def timestep_embedding(ts, mult, dim):
    """ts [n] -> [n][dim]: [cos(t f_k) | sin(t f_k)], t = ts * mult (LTXTimestepEmbedding.swift:17-54)"""
    arg = (np.asarray(ts, F64) * f32(mult))[:, None] * timestep_frequencies(dim)[None, :]
    return np.concatenate([np.cos(arg), np.sin(arg)], axis=1)


def timestep_embedding_f32(ts, mult, dim):
    """The same five operations (ts * mult, k / half, the product with -ln 10000, exp, the product with t) and the cosine / sine, each
    rounded to FLOAT32: the measure of what f32 arithmetic alone costs against `timestep_embedding`."""
    t = np.asarray(ts, np.float32) * np.float32(mult)
    arg = t[:, None] * timestep_frequencies(dim, np.float32)[None, :]
    assert arg.dtype == np.float32
    return np.concatenate([np.cos(arg), np.sin(arg)], axis=1)


def i2v_rowmap(B, T, first, G):
    """row_map[b][t] = b*G + (1 for the first `first` tokens - frame 0, whose timestep is 0 - else 0)"""
    return (np.arange(B)[:, None] * G + (np.arange(T)[None, :] < first)).astype(np.int32)


def i2v_timesteps(B, G, sigma):
    """B rows of [sigma, 0, .., 0] (G entries: group 0 is the noisy one), then B audio timesteps sigma"""
    video = np.zeros((B, G))
    video[:, 0] = f32(sigma)
    return np.concatenate([video.reshape(-1), np.full(B, f32(sigma))])


def gemma_mask_scan(mask):
    """mask [B][T] -> (key_start [B], status [B]): the index of the first 1 (T without one); 1 when the row is 0..0 1..1 with at least
    one 1 and holds nothing but 0 and 1"""
    mask = np.asarray(mask)
    T = mask.shape[1]
    one = mask == 1
    first = np.where(one.any(axis=1), one.argmax(axis=1), T)
    form = (np.arange(T)[None, :] >= first[:, None]) == one
    ok = form.all(axis=1) & one.any(axis=1) & np.isin(mask, (0, 1)).all(axis=1)
    return first.astype(np.int32), ok.astype(np.int32)


def sp_vt_interleave(g):
    """gathered [N][D][Tn] -> V^T [D][N*Tn]: rank r's keys at columns r*Tn .."""
    g = np.asarray(g, F64)
    N, D, Tn = g.shape
    return g.transpose(1, 0, 2).reshape(D, N * Tn)


# ---- VAE encoder ----
def enc_patchify(pixels):
    """pixels [3][T][H][W] -> [T][H/4][W/4][64]: channel c*16 + pw*4 + ph (pW before pH, VideoEncoder.swift:25-31), 48 .. 63 zero"""
    px = np.asarray(pixels, F64)
    _, T, H, W = px.shape
    v = px.reshape(3, T, H // 4, 4, W // 4, 4).transpose(1, 2, 4, 0, 5, 3).reshape(T, H // 4, W // 4, 48)  # (t, h4, w4, c, pw, ph)
    return np.concatenate([v, np.zeros((T, H // 4, W // 4, 16))], axis=-1)


def space_to_depth(x, ft, fh, fw):
    """x [T][H][W][C] -> [T2][H/fh][W/fw][C*S], channel c*S + (it*fh + ih)*fw + iw; T is padded in FRONT with copies of frame 0 to a
    multiple of ft (VAESpaceToDepthDownsample3d, VideoEncoder.swift:146-167)"""
    x = np.asarray(x, F64)
    pad = (-x.shape[0]) % ft
    x = np.concatenate([np.repeat(x[:1], pad, axis=0), x], axis=0)
    T, H, W, C = x.shape
    v = x.reshape(T // ft, ft, H // fh, fh, W // fw, fw, C).transpose(0, 2, 4, 6, 1, 3, 5)  # (t2, h2, w2, c, it, ih, iw)
    return v.reshape(T // ft, H // fh, W // fw, C * ft * fh * fw)


def enc_s2d_residual(conv, x, ft, fh, fw):
    """s2d(conv) + the mean over groups of G adjacent channels of s2d(x), G = Cx*S / Cout. Returns (out, conv part, group mean of |x|)."""
    c = space_to_depth(conv, ft, fh, fw)
    s = space_to_depth(x, ft, fh, fw)
    Cout = c.shape[-1]
    grouped = s.reshape(s.shape[:-1] + (Cout, s.shape[-1] // Cout))
    return c + grouped.mean(axis=-1), c, np.abs(grouped).mean(axis=-1)


def enc_finish(z, C, mean=None, std=None):
    """z [P][ldz] -> [C][P] of the first C columns, (z - mean[c]) / std[c] with statistics (LTXPipeline.swift:1920-1927)"""
    v = np.asarray(z, F64)[:, :C].T
    if mean is not None:
        v = (v - np.asarray(mean, F64)[:, None]) / np.asarray(std, F64)[:, None]
    return v


# ---- audio row passes: (interior values, (rows, cols) of the haloed plane, (row, col) of the interior's first element) ----
EPS_AUDIO_PN = float(np.float32(1e-6))


def audio_pn_pad(x, mode):
    """x [H][W][C]: mode 0 SiLU(x / sqrt(mean_c(x^2) + 1e-6)) (AudioVAE.swift:23-26, :146-152), mode 1 x; the operand of the
    height-causal 3x3 conv: two zero rows above, one below, one zero column on each side."""
    x = np.asarray(x, F64)
    H, W, _ = x.shape
    v = silu(x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + EPS_AUDIO_PN)) if mode == 0 else x
    return v, (H + 3, W + 2), (2, 1)


def audio_upsample_pad(x):
    """nearest 2x on both axes; the conv that follows drops its first output row, so ONE zero row on top (AudioVAE.swift:178-198)"""
    x = np.asarray(x, F64)
    H, W, _ = x.shape
    return np.repeat(np.repeat(x, 2, axis=0), 2, axis=1), (2 * H + 2, 2 * W + 2), (1, 1)


def audio_denorm_pad(latent, mean, std):
    """latent [Cl][T][Wl] * std[c*Wl + w] + mean[c*Wl + w] -> [T][Wl][Cl] (AudioVAE.swift:415-434)"""
    lat = np.asarray(latent, F64)
    Cl, T, Wl = lat.shape
    v = lat * np.asarray(std, F64).reshape(Cl, 1, Wl) + np.asarray(mean, F64).reshape(Cl, 1, Wl)
    return v.transpose(1, 2, 0), (T + 3, Wl + 2), (2, 1)


def audio_mel_pack(mel):
    """mel [2][T][M] -> [T][2*M], column c*M + m (Vocoder.swift:220-229)"""
    mel = np.asarray(mel, F64)
    return mel.transpose(1, 0, 2).reshape(mel.shape[1], -1)


def audio_mean3_act(a, b, c, slope):
    """leaky((a + b + c) / 3, slope) (Vocoder.swift:242-250 and the consumer's LeakyReLU); a mean of +-0 takes the >= 0 branch"""
    s = (np.asarray(a, F64) + np.asarray(b, F64) + np.asarray(c, F64)) / 3.0
    return np.where(s >= 0, s, s * f32(slope))
