"""Device buffers with a guarded tail, and the comparisons of the helper-pass tests (test_helper_passes_gpu.py,
test_row_passes_rest_gpu.py): every output is allocated with slack behind its valid extent and filled with a sentinel that no case
produces; reading it back checks that the slack kept the sentinel."""
import numpy as np
import torch

import helper_pass_ref as ref

SENTINEL_F32 = -24680.125      # an f32 value that no case produces
SENTINEL_BITS = 0x5A5A         # bf16 bit pattern (about 1.5e13) that no case produces


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def dev_bf16(x):
    """bf16 VALUES (any float array) -> device bf16 tensor"""
    return torch.from_numpy(ref.bf16_bits(x).view(np.int16)).cuda().view(torch.bfloat16)


def out_f32(n, slack):
    return torch.full((n + slack,), SENTINEL_F32, dtype=torch.float32, device="cuda")


def out_bf16(n, slack):
    return torch.full((n + slack,), SENTINEL_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def host_f32(t, n, shape=None):
    """The first n elements as float64 (exact), after checking that everything behind them kept the sentinel."""
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert a.size > n and np.all(a[n:] == np.float32(SENTINEL_F32)), "wrote past the valid extent"
    return a[:n].reshape(shape or (n,))


def host_bf16(t, n, shape=None):
    torch.cuda.synchronize()
    b = t.view(torch.int16).cpu().numpy().view(np.uint16)
    assert b.size > n and np.all(b[n:] == SENTINEL_BITS), "wrote past the valid extent"
    return b[:n].reshape(shape or (n,))


def same_f32_bits(got, want):
    return np.array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float64).astype(np.float32).view(np.uint32))


def exact_f32(x):
    """x as f32, asserting that nothing is lost: the expected value of a bit-equal case"""
    y = np.asarray(x, np.float64).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x)
    return y


def bf16_rule(got_bits, want_f64, what):
    want = ref.bf16(want_f64)
    got = ref.from_bf16_bits(got_bits)
    dist = np.abs(got - want)
    limit = ref.bf16_ulp(want) + 1e-6
    worst = float((dist / limit).max())
    frac = float((got != want).mean())
    print(f"{what}: worst distance {worst:.3f} of (1 bf16 ulp + 1e-6), {frac:.2e} of the elements differ (cap 1e-3)")
    return worst <= 1.0 and frac <= 1e-3


def report(what, err, bound):
    """Largest error / bound ratio of a derived bound; printed before the caller asserts it."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: worst error {float(err.max()):.3e}, at the tightest element {float(err[i]):.3e} against a bound of {float(bound[i]):.3e} "
          f"(largest error / bound = {ratio:.3f})")
    return bool(np.all(err <= bound))
