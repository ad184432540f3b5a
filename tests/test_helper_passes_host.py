"""Host-side checks of what tests/test_row_passes_rest_gpu.py leans on (no GPU):
  * the `bf16_rule` cap of 1e-3 differing elements is a condition, not a measurement: a numpy FLOAT32 replay of audio_pn_pad mode 0 and
    of audio_mean3_act, on exactly the inputs the GPU tests use, rounds to another bf16 value than the float64 reference in under 1e-4
    of the elements - the cap leaves at least 10x room for the reference alone;
  * every new restatement of tests/helpers/helper_pass_ref.py against a brute-force loop over its output elements on the smallest
    shapes, and the register plan against plans worked out by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import helper_pass_ref as ref  # noqa: E402
import row_pass_cases as cases  # noqa: E402


def differing(replay_f32, want_f64):
    return int((ref.bf16(replay_f32.astype(np.float64)) != ref.bf16(want_f64)).sum()), replay_f32.size


def test_f32_replay_of_pn_pad_rounds_like_float64():
    diff = total = 0
    for H, W, C in cases.PN_PAD_SHAPES:
        x = cases.pn_pad_input(H, W, C)
        ss = (x * x).sum(axis=-1, keepdims=True, dtype=np.float32)
        v = x * (np.float32(1.0) / np.sqrt(ss / np.float32(C) + np.float32(1e-6)))
        replay = v / (np.float32(1.0) + np.exp(-v))
        assert replay.dtype == np.float32
        d, n = differing(replay, ref.audio_pn_pad(x, 0)[0])
        diff, total = diff + d, total + n
    print(f"audio_pn_pad: an f32 replay differs from bf16(float64) in {diff} of {total} elements ({diff / total:.2e})")
    assert diff / total < 1e-4


def test_f32_replay_of_mean3_act_rounds_like_float64():
    diff = total = 0
    for rows, C, _ in cases.MEAN3_SHAPES:
        a, b, c = cases.mean3_inputs(rows, C)
        for slope in cases.MEAN3_SLOPES:
            s = (a + b + c) / np.float32(3.0)
            replay = np.where(s >= 0, s, s * np.float32(slope))
            assert replay.dtype == np.float32
            d, n = differing(replay, ref.audio_mean3_act(a, b, c, np.float32(slope)))
            diff, total = diff + d, total + n
    print(f"audio_mean3_act: an f32 replay differs from bf16(float64) in {diff} of {total} elements ({diff / total:.2e})")
    assert diff / total < 1e-4


def test_bf16_rne_bits_is_bf16_where_both_are_defined():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-30, 30, 20000), [1.00390625, 1.01171875, 1.99999988, 0.0]]).astype(np.float32)
    x = x[(np.abs(x) >= 2.0 ** -126) | (x == 0)]
    assert np.array_equal(ref.bf16_rne_bits(x), ref.bf16_bits(ref.bf16(x)))
    bits = lambda u: np.array(u, np.uint32).view(np.float32)
    # below the normal range, at the top and at the zeros: by hand
    assert ref.bf16_rne_bits(bits([0x00008000, 0x00018000, 0x00008001, 0x007F8000, 0x7F7F8000, 0x7F800000, 0x80000000, 0x00000001])).tolist() == [
        0x0000, 0x0002, 0x0001, 0x0080, 0x7F80, 0x7F80, 0x8000, 0x0000]


def test_register_plan_by_hand_and_by_loop():
    assert ref.register_plan([[1]]).tolist() == [[0]] and ref.register_plan([[0]]).tolist() == [[-1]]
    assert ref.register_plan([[0, 0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0, 0, 0], [1] * 9]).tolist() == [
        [4, 5, 6, 7, 8, -1, -1, -1, -1],   # left padding: the 5 tokens move to the front, registers fill the rest
        [-1, -1, -1, -1, -1, 5, 6, 7, 8],  # right padding: the reversed mask keeps the LAST 4 positions, which hold padded tokens
        [0, 1, 2, 3, 4, 5, 6, 7, 8]]
    assert ref.register_plan([[0] * 5, [1, 0, 1, 1, 0]]).tolist() == [[-1] * 5, [-1, 2, 3, -1, 4]]
    rng = np.random.default_rng(1)
    mask = rng.integers(0, 2, (20, 7))
    for m, got in zip(mask, ref.register_plan(mask)):
        order = [t for t in range(7) if m[t]] + [t for t in range(7) if not m[t]]
        assert got.tolist() == [order[p] if m[6 - p] else -1 for p in range(7)]


def test_register_gather_by_loop():
    rng = np.random.default_rng(2)
    B, T, D, R = 2, 5, 3, 2
    enc, reg = rng.standard_normal((B, T, D)), rng.standard_normal((R, D))
    src = np.array([[2, -1, -1, 0, 0], [-1, -1, -1, -1, 4]])
    got = ref.register_gather(enc, reg, src)
    for b in range(B):
        for p in range(T):
            assert np.array_equal(got[b, p], enc[b, src[b, p]] if src[b, p] >= 0 else reg[p % R])


def test_enc_patchify_by_loop():
    T, H, W = 2, 4, 8
    px = np.random.default_rng(3).standard_normal((3, T, H, W))
    got = ref.enc_patchify(px)
    assert got.shape == (T, 1, 2, 64) and not got[..., 48:].any()
    for t in range(T):
        for w4 in range(2):
            for c in range(3):
                for pw in range(4):
                    for ph in range(4):
                        assert got[t, 0, w4, c * 16 + pw * 4 + ph] == px[c, t, ph, 4 * w4 + pw]


def test_enc_s2d_residual_by_loop():
    rng = np.random.default_rng(4)
    for (ft, fh, fw), T in (((2, 1, 1), 3), ((1, 2, 2), 2), ((2, 2, 2), 1), ((2, 2, 2), 4)):
        S, H, W, Cc, Cx = ft * fh * fw, 2, 4, 1, 2
        Cout, G = Cc * S, 2
        conv, x = rng.standard_normal((T, H, W, Cc)), rng.standard_normal((T, H, W, Cx))
        got, _, _ = ref.enc_s2d_residual(conv, x, ft, fh, fw)
        pad = (-T) % ft
        assert got.shape == ((T + pad) // ft, H // fh, W // fw, Cout)

        def s2d(src, t2, h2, w2, cs):  # channel cs = c * S + (it * fh + ih) * fw + iw; frame -1 of an odd T is frame 0
            c, sub = divmod(cs, S)
            it, rest = divmod(sub, fh * fw)
            ih, iw = divmod(rest, fw)
            return src[max(0, t2 * ft + it - pad), h2 * fh + ih, w2 * fw + iw, c]

        for idx in np.ndindex(got.shape):
            t2, h2, w2, co = idx
            want = s2d(conv, t2, h2, w2, co) + sum(s2d(x, t2, h2, w2, co * G + g) for g in range(G)) / G
            assert abs(got[idx] - want) <= 1e-15


def test_enc_finish_and_small_layouts_by_loop():
    rng = np.random.default_rng(5)
    z, mean, std = rng.standard_normal((4, 7)), rng.standard_normal(5), rng.uniform(0.5, 2, 5)
    got = ref.enc_finish(z, 5, mean, std)
    for c in range(5):
        for p in range(4):
            assert got[c, p] == (z[p, c] - mean[c]) / std[c] and ref.enc_finish(z, 5)[c, p] == z[p, c]
    g = rng.standard_normal((3, 2, 8))
    vt = ref.sp_vt_interleave(g)
    assert all(vt[d, r * 8 + t] == g[r, d, t] for r in range(3) for d in range(2) for t in range(8))
    mel = rng.standard_normal((2, 3, 4))
    packed = ref.audio_mel_pack(mel)
    assert all(packed[t, c * 4 + m] == mel[c, t, m] for c in range(2) for t in range(3) for m in range(4))
    lat, mean, std = rng.standard_normal((3, 2, 5)), rng.standard_normal(15), rng.uniform(0.5, 2, 15)
    v, plane, at = ref.audio_denorm_pad(lat, mean, std)
    assert plane == (5, 7) and at == (2, 1)
    assert all(v[t, w, c] == lat[c, t, w] * std[c * 5 + w] + mean[c * 5 + w] for c in range(3) for t in range(2) for w in range(5))
    x = rng.standard_normal((2, 3, 4))
    up, plane, at = ref.audio_upsample_pad(x)
    assert plane == (6, 8) and at == (1, 1)
    assert all(np.array_equal(up[u, w], x[u // 2, w // 2]) for u in range(4) for w in range(6))
    pn, plane, at = ref.audio_pn_pad(x, 0)
    assert plane == (5, 5) and at == (2, 1)
    for h in range(2):
        for w in range(3):
            y = x[h, w] / np.sqrt(np.mean(x[h, w] ** 2) + ref.EPS_AUDIO_PN)
            assert np.allclose(pn[h, w], y / (1 + np.exp(-y)), rtol=1e-15, atol=0)
    assert np.array_equal(ref.audio_pn_pad(x, 1)[0], x)
    table, te = rng.standard_normal((4, 3)), rng.standard_normal((4, 3))
    mods = ref.vae_make_mods(table, te)
    assert all(mods[r, c] == table[r, c] + te[r, c] + (r % 2) for r in range(4) for c in range(3))
    assert np.array_equal(ref.vae_make_mods(table), table + np.array([0, 1, 0, 1.0])[:, None])


def test_integer_plans_by_hand():
    assert ref.i2v_rowmap(2, 4, 1, 2).tolist() == [[1, 0, 0, 0], [3, 2, 2, 2]]
    assert ref.i2v_timesteps(2, 3, 0.5).tolist() == [0.5, 0, 0, 0.5, 0, 0, 0.5, 0.5]
    start, status = ref.gemma_mask_scan([[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0], [0, 1, 0, 1], [0, 2, 1, 1], [0, 0, 0, 1]])
    assert start.tolist() == [2, 0, 4, 0, 1, 2, 3] and status.tolist() == [1, 1, 0, 0, 0, 0, 1]


def test_elementwise_references_by_hand():
    a, b = np.array([8.0, -4.0]), np.array([4.0, 12.0])
    assert ref.cfg_combine(a, b, 3.0).tolist() == [4 + 2 * (4 - 8), 12 + 2 * (12 + 4)]     # cond + 2 (cond - uncond)
    assert ref.lincomb(a, b, 2.0, -0.5).tolist() == [14.0, -14.0]
    assert ref.axpby(a, b, 0.5, 2.0).tolist() == [2 * 8 + 0.5 * 4, 2 * -4 + 0.5 * -16]
    assert ref.ge(a, b, 0.25).tolist() == [0.25 * 4 + 4, 0.25 * -16 + 12]
    assert ref.clip01([-3, -1, -0.5, 0, 0.5, 1, 3]).tolist() == [0, 0, 0.25, 0.5, 0.75, 1, 1]
    bias = ref.mask_to_bias([1, 0])
    assert bias.tolist() == [0.0, -10000.0] and not np.signbit(bias[0])
    emb = ref.timestep_embedding(np.array([0.0, 0.5], np.float32), 1000.0, 4)
    assert emb[0].tolist() == [1, 1, 0, 0]
    assert np.allclose(emb[1], [np.cos(500.0), np.cos(5.0), np.sin(500.0), np.sin(5.0)], rtol=0, atol=1e-12)  # f = 1, 10000^-1/2
