"""Plain numpy float64 restatements of the helper passes of csrc/elementwise.h (guidance, scheduler, VAE, latent upscaler, connector),
written from the formulas in that header and the reference seams it cites, one array expression per formula. Inputs are taken as they
are (f32 or bf16 VALUES held in any float array) and widened to float64; nothing here rounds, except `bf16*` (the output format of the
bf16 passes) and `set_frame0_f32` (whose contract is a float32 replay). Scalars that a kernel receives as f32 must be passed as the
f32 value (np.float32(0.4), not 0.4): `f32()` does that."""
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


def fe_norm_concat(hidden, mask, mean, range_eps, padding_right):
    """out[b][t][d*S + l] = valid ? 8*(x - mean[l][b]) / range_eps[l][b] : 0   -> [B][T][D*S] (before the rounding to bf16)"""
    h = np.asarray(hidden, F64)
    S, B, T, D = h.shape
    valid = fe_valid(mask, padding_right)
    v = 8.0 * (h - np.asarray(mean, F64)[:, :, None, None]) / np.asarray(range_eps, F64)[:, :, None, None]
    v = np.where(valid[None, :, :, None], v, 0.0)
    return v.transpose(1, 2, 3, 0).reshape(B, T, D * S)
