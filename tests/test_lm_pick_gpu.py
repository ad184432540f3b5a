"""lm_pick_kernel (csrc/elementwise.hip) through ltx_op_lm_pick: repetition penalty + argmax on the device, compared EXACTLY to the
numpy restatement (tests/helpers/gemma_decode_ref.py): the token, the penalised logits left in the buffer, and the appended history."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_decode_ref as dec  # noqa: E402

pytestmark = pytest.mark.gpu
VOCAB = 262208


def run(ctx, logits, generated=(), context=64, penalty=1.0):
    """-> (token, logits after the call, history after the call)."""
    n = len(generated)
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    hist = torch.full((n + 2,), -5, dtype=torch.int32, device="cuda")
    hist[:n] = torch.tensor(list(generated), dtype=torch.int32)
    out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ctx.op_lm_pick(lg, out, hist=hist, n_gen=n, context=context, penalty=penalty)
    torch.cuda.synchronize()
    return int(out.item()), lg.cpu().numpy(), hist.cpu().numpy()


def check(ctx, logits, generated=(), context=64, penalty=1.0):
    tok, after, hist = run(ctx, logits, generated, context, penalty)
    want = dec.penalize(logits, list(generated), context, penalty)
    assert np.array_equal(after, want)  # bit for bit: the division is IEEE
    assert tok == dec.pick(want)
    assert list(hist[:len(generated)]) == list(generated) and hist[len(generated)] == tok and hist[-1] == -5
    return tok


@pytest.mark.parametrize("vocab", [1, 3, 4, 5, 1000, 4097, VOCAB])
def test_constructed_ties_go_to_the_lowest_index(gpu_ctx, vocab):
    """All equal; a tie between the first and the last index; ties inside one 16-byte vector, across threads and across waves; the
    maximum alone at the last index (the scalar tail when vocab % 4 != 0)."""
    flat = np.full(vocab, -3.5, np.float32)
    assert check(gpu_ctx, flat) == 0
    l = flat.copy()
    l[[0, vocab - 1]] = 2.0
    assert check(gpu_ctx, l) == 0
    l = flat.copy()
    l[vocab - 1] = 2.0
    assert check(gpu_ctx, l) == vocab - 1
    if vocab >= 1000:
        rng = np.random.default_rng(vocab)
        for _ in range(4):
            l = rng.standard_normal(vocab).astype(np.float32)
            idx = np.sort(rng.choice(vocab, 6, replace=False))
            l[idx] = 9.0
            l[idx[0] + 1 if idx[0] + 1 < vocab and idx[0] + 1 not in idx else idx[0]] = 9.0  # and its neighbour in the same vector
            assert check(gpu_ctx, l) == idx[0]
        l = rng.standard_normal(vocab).astype(np.float32)
        check(gpu_ctx, l)


def test_penalty_on_positive_negative_and_zero_logits(gpu_ctx):
    l = np.array([0.0, 3.0, -3.0, 2.9, -0.0, 1e-30, -1e30, 2.0], np.float32)
    for p in (1.1, 1.5, 3.0, 0.5):
        # 3.0 / p falls below 2.9 for p >= 1.1: the pick moves; 0 and -0 stay; the negative grows
        tok = check(gpu_ctx, l, generated=[1, 2, 0, 4, 5, 6], penalty=p)
        assert tok == (3 if p > 1 else 1)
    assert check(gpu_ctx, l, generated=[1], penalty=1.0) == 1  # p == 1: nothing applied
    assert check(gpu_ctx, l, generated=[], penalty=2.0) == 1   # nothing generated: nothing applied


def test_duplicate_ids_are_penalised_once(gpu_ctx):
    rng = np.random.default_rng(2)
    l = (rng.standard_normal(1000) * 4).astype(np.float32)
    gen = [7, 7, 7, 500, 7, 500, 999, 0, 999, 7]
    tok, after, _ = run(gpu_ctx, l, gen, context=64, penalty=1.3)
    assert after[7] == (l[7] / np.float32(1.3) if l[7] > 0 else l[7] * np.float32(1.3))
    check(gpu_ctx, l, gen, context=64, penalty=1.3)
    # the maximum itself, repeated: penalised once it loses to the runner-up only if one division is enough
    l2 = np.zeros(1000, np.float32)
    l2[10], l2[20] = 4.0, 3.0
    assert check(gpu_ctx, l2, [10, 10, 10], penalty=1.2) == 10   # 4 / 1.2 = 3.33 > 3; three divisions would give 2.31
    assert check(gpu_ctx, l2, [10, 10, 10], penalty=1.5) == 20


def test_context_window(gpu_ctx):
    """Context longer than the generated count takes all of it; a shorter one only the newest entries; ids outside the vocabulary are
    passed over; a history longer than one pass of the workgroup's threads."""
    rng = np.random.default_rng(4)
    l = (rng.standard_normal(5000) * 3).astype(np.float32)
    top = int(np.argmax(l))
    gen = [top, 3, 4, 5]
    assert check(gpu_ctx, l, gen, context=64, penalty=100.0) != top   # 4 generated, context 64
    assert check(gpu_ctx, l, gen, context=3, penalty=100.0) == top    # the window no longer reaches it
    assert check(gpu_ctx, l, gen, context=0, penalty=100.0) == top
    check(gpu_ctx, l, [top, -1, 5000, 2 ** 30], context=64, penalty=2.0)
    long_gen = [int(t) for t in rng.integers(0, 5000, 1500)]
    check(gpu_ctx, l, long_gen, context=1400, penalty=1.7)


def test_full_vocabulary_with_the_defaults(gpu_ctx):
    rng = np.random.default_rng(6)
    l = (rng.standard_normal(VOCAB) * 5).astype(np.float32)
    gen = [int(t) for t in np.argsort(-l)[:40]] + [int(t) for t in rng.integers(0, VOCAB, 60)]
    check(gpu_ctx, l, gen, context=64, penalty=1.1)


def test_refusals(gpu_ctx, ltx):
    lg = torch.zeros(16, device="cuda")
    out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    hist = torch.zeros(4, dtype=torch.int32, device="cuda")
    for bad in (dict(logits=None, vocab=16), dict(out=None), dict(vocab=0), dict(logits=lg[1:]), dict(n_gen=2), dict(n_gen=-1, hist=hist),
                dict(context=-1), dict(penalty=0.0), dict(penalty=-1.0)):
        kw = {**dict(logits=lg, out=out, hist=None, n_gen=0, context=64, penalty=1.0), **bad}
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.op_lm_pick(**kw)
        assert e.value.code == 2, bad
    torch.cuda.synchronize()
    assert int(out.item()) == -7
