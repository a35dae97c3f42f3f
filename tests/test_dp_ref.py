"""Differential privacy for secure aggregation on the CPU: the binomial-noise
specification (an independent recomputation, offset slicing, deterministic
moments), exactness of noise + masks in Z/2^32 through the public API,
validation, and clip_factor / sum_squares."""
import functools
import hashlib
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from rayfed_amd.ops import secagg_ref as ref  # noqa: E402
from rayfed_amd.parallel import (  # noqa: E402
    BinomialNoise,
    SecAggSession,
    aggregate,
    clip_factor,
    sum_squares,
)

WORDS = [1, 2, 4, 8, 16]
KEY = hashlib.sha256(b"n").digest()
ROUND = 7
NMOM = 65536
BIG_ROUND = (5 << 32) | 0x9ABCDEF1
SECRET = b"dp-unit-test-secret"


@functools.lru_cache(maxsize=None)
def _noise(words):
    """binomial_noise(KEY, ROUND, 0, NMOM, words, 1), computed once."""
    z = ref.binomial_noise(KEY, ROUND, 0, NMOM, words, 1)
    z.setflags(write=False)
    return z


def _independent(key, rnd, n, words, step, third_word):
    """The definition, recomputed from chacha20_blocks + np.bitwise_count."""
    nblocks = (n * words + 15) // 16
    blk = ref.chacha20_blocks(
        key, 0, (rnd & 0xFFFFFFFF, rnd >> 32, third_word), nblocks)
    w = blk.reshape(-1)[: n * words].reshape(n, words)
    pop = np.bitwise_count(w).astype(np.int64).sum(axis=1)
    return ((pop - 16 * words) * step % (1 << 32)).astype(np.uint32)


# ------------------------------------------------------- noise definition
@pytest.mark.parametrize("words", WORDS)
def test_noise_matches_independent_computation(words):
    n = 1000
    for rnd, step in ((ROUND, 1), (BIG_ROUND, 1000), (BIG_ROUND, 1 << 20)):
        got = ref.binomial_noise(KEY, rnd, 0, n, words, step)
        assert got.dtype == np.uint32 and got.shape == (n,)
        assert np.array_equal(got, _independent(KEY, rnd, n, words, step, 1))
        # domain separation: the pair-mask nonce (third word 0) differs
        assert not np.array_equal(
            got, _independent(KEY, rnd, n, words, step, 0))


@pytest.mark.parametrize("words", WORDS)
def test_noise_offset_slicing(words):
    full = ref.binomial_noise(KEY, ROUND, 0, 132, words, 3)
    part = ref.binomial_noise(KEY, ROUND, 32, 100, words, 3)
    assert np.array_equal(part, full[32:132])
    assert np.array_equal(full, 3 * _noise(words)[:132])


def test_mask_offset_slicing_with_noise():
    parties = ["alice", "bob", "carol"]
    s = SecAggSession.from_shared_secret(parties, "bob", SECRET)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(132, generator=g)
    for words in WORDS:
        noise = BinomialNoise(KEY, words=words, step=5)
        whole = s.mask(x, round=ROUND, weight=0.5, noise=noise)
        part = s.mask(x[32:], round=ROUND, weight=0.5, offset=32, noise=noise)
        assert torch.equal(part, whole[32:])


# ---------------------------------------------------------------- moments
@pytest.mark.parametrize("words", WORDS)
def test_noise_moments(words):
    """Deterministic (fixed key): 4-standard-error bounds on the mean and
    the variance of step*(Bin(32W, 1/2) - 16W) at step 1, and the hard
    bound.  Measured with this reference: worst |mean| 1.8 standard errors,
    worst variance deviation 1.05 % against the 2.2 % bound."""
    z = _noise(words).view(np.int32).astype(np.float64)
    assert abs(z.mean()) <= 4 * math.sqrt(8 * words / NMOM)
    assert abs(z.var() / (8 * words) - 1) <= 4 * math.sqrt(2 / NMOM)
    assert np.abs(z).max() <= 16 * words


# -------------------------------------------------------------- exactness
@pytest.mark.parametrize("words,step", [(1, 1), (4, 1000), (16, 1 << 20)])
def test_mask_noise_ref_minus_mask_ref_is_the_noise(words, step):
    n = 333
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(n, generator=g) * 50).numpy()
    keys = [hashlib.sha256(b"k%d" % i).digest() for i in range(3)]
    signs = [1, -1, 1]
    a = ref.mask_noise_ref(x, 0.3, 16, keys, signs, BIG_ROUND, 16, KEY,
                           words, step)
    b = ref.mask_ref(x, 0.3, 16, keys, signs, BIG_ROUND, 16)
    assert a.dtype == np.int32
    assert np.array_equal(a.view(np.uint32) - b.view(np.uint32),
                          ref.binomial_noise(KEY, BIG_ROUND, 16, n, words,
                                             step))


def test_three_parties_one_dropped_aggregate_is_sum_plus_survivor_noise():
    parties = ["alice", "bob", "carol"]
    dropped = ["bob"]
    survivors = ["alice", "carol"]
    n = 1000
    rnd = 21
    sess = {p: SecAggSession.from_shared_secret(parties, p, SECRET)
            for p in parties}
    noises = {p: BinomialNoise(hashlib.sha256(p.encode()).digest(), 4, 37)
              for p in parties}
    w = {"alice": 0.5, "bob": 0.25, "carol": 0.125}
    ups = {}
    for i, p in enumerate(parties):
        g = torch.Generator().manual_seed(60 + i)
        ups[p] = torch.randn(n, generator=g) * 3
    masked = {p: sess[p].mask(ups[p], round=rnd, weight=w[p], noise=noises[p])
              for p in survivors}
    revealed = {p: sess[p].reveal(dropped) for p in survivors}
    out = aggregate(masked, parties, round=rnd, revealed=revealed)
    acc = np.zeros(n, dtype=np.uint32)
    for p in survivors:
        acc += ref.quantize(ups[p].numpy(), w[p], 16).view(np.uint32)
        acc += ref.binomial_noise(noises[p].key, rnd, 0, n, 4, 37)
    want = acc.view(np.int32).astype(np.float32) * np.float32(2.0 ** -16)
    assert np.array_equal(out.numpy(), want)
    # the noise is really there, and bounded by max_abs(2 contributors)
    plain = {p: sess[p].mask(ups[p], round=rnd, weight=w[p])
             for p in survivors}
    out0 = aggregate(plain, parties, round=rnd, revealed=revealed)
    diff = (out - out0).abs().max().item()
    assert 0 < diff <= noises["alice"].max_abs(16, contributors=2)


def test_noise_none_is_the_plain_path():
    s = SecAggSession.from_shared_secret(["a", "b", "c"], "a", SECRET)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(100, generator=g).to(torch.bfloat16)
    keys = [s.reveal([p])[p] for p in ("b", "c")]
    want = ref.mask_ref(x.float().numpy(), 0.7, 16, keys, [1, 1], ROUND, 16)
    got = s.mask(x, round=ROUND, weight=0.7, offset=16, noise=None)
    assert np.array_equal(got.numpy(), want)
    assert torch.equal(got, s.mask(x, round=ROUND, weight=0.7, offset=16))


# ------------------------------------------------------------- validation
@pytest.mark.parametrize("words", [3, 32, 0, -4, 4.0, True])
def test_bad_words_rejected(words):
    with pytest.raises(ValueError):
        ref.binomial_noise(KEY, ROUND, 0, 16, words, 1)
    with pytest.raises(ValueError):
        BinomialNoise(KEY, words=words)


@pytest.mark.parametrize("step", [0, (1 << 20) + 1, -1, 1.5])
def test_bad_step_rejected(step):
    with pytest.raises(ValueError):
        ref.binomial_noise(KEY, ROUND, 0, 16, 4, step)
    with pytest.raises(ValueError):
        BinomialNoise(KEY, step=step)


def test_bad_key_and_offset_rejected():
    with pytest.raises(ValueError):
        ref.binomial_noise(KEY[:31], ROUND, 0, 16, 4, 1)
    with pytest.raises(ValueError):
        BinomialNoise(KEY[:31])
    with pytest.raises(ValueError):
        BinomialNoise("k" * 32)
    with pytest.raises(ValueError):
        ref.binomial_noise(KEY, ROUND, 8, 16, 4, 1)
    with pytest.raises(ValueError):
        ref.binomial_noise(KEY, -1, 0, 16, 4, 1)
    s = SecAggSession.from_shared_secret(["a", "b"], "a", SECRET)
    with pytest.raises(ValueError):
        s.mask(torch.zeros(16), round=0, offset=8, noise=BinomialNoise(KEY))
    with pytest.raises(ValueError):
        s.mask(torch.zeros(16), round=0, noise=(KEY, 4, 1))


@pytest.mark.parametrize("words", WORDS)
def test_counter_limit(words):
    top = (1 << 36) // words - 16  # (top + 16) * W == 2^36: accepted
    z = ref.binomial_noise(KEY, ROUND, top, 16, words, 1)
    assert z.shape == (16,)
    with pytest.raises(ValueError):  # (top + 17) * W == 2^36 + W
        ref.binomial_noise(KEY, ROUND, top, 17, words, 1)
    with pytest.raises(ValueError):
        ref.binomial_noise(KEY, ROUND, top + 16, 1, words, 1)
    s = SecAggSession.from_shared_secret(["a", "b"], "a", SECRET)
    noise = BinomialNoise(KEY, words=words)
    y = s.mask(torch.zeros(16), round=ROUND, offset=top, noise=noise)
    want = ref.mask_noise_ref(np.zeros(16, np.float32), 1.0, 16,
                              [s.reveal(["b"])["b"]], [1], ROUND, top, KEY,
                              words, 1)
    assert np.array_equal(y.numpy(), want)
    with pytest.raises(ValueError):
        s.mask(torch.zeros(17), round=ROUND, offset=top, noise=noise)
    if words > 1:  # the plain path keeps its own, wider rule
        s.mask(torch.zeros(17), round=ROUND, offset=top)


def test_binomial_noise_object():
    nz = BinomialNoise(KEY, words=8, step=100)
    assert nz.std(16) == 100 * math.sqrt(64) / 65536
    assert nz.std(16, contributors=4) == 100 * math.sqrt(256) / 65536
    assert nz.max_abs(16) == 16 * 8 * 100 / 65536
    assert nz.max_abs(10, contributors=3) == 16 * 8 * 100 * 3 / 1024
    with pytest.raises(AttributeError):
        nz.step = 2  # immutable
    assert KEY.hex() not in repr(nz) and repr(KEY) not in repr(nz)
    d = BinomialNoise(KEY)
    assert (d.words, d.step) == (4, 1)
    with pytest.raises(ValueError):
        nz.std(31)
    with pytest.raises(ValueError):
        nz.max_abs(16, contributors=0)
    a, b = BinomialNoise.fresh(2, 9), BinomialNoise.fresh(2, 9)
    assert (a.words, a.step, len(a.key)) == (2, 9, 32) and a.key != b.key


# ------------------------------------------------ clip_factor, sum_squares
def test_sum_squares_reference_and_dtypes():
    assert ref.sum_squares_ref(np.zeros(0, np.float32)) == 0.0
    assert ref.sum_squares_ref(np.array([3, 4], np.float32)) == 25.0
    assert ref.sum_squares_ref(np.full(4, 1e30, np.float32)) == pytest.approx(
        4 * float(np.float32(1e30)) ** 2, rel=1e-15)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4101, generator=g)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        xd = x.to(dt)
        exact = math.fsum(float(v) ** 2 for v in xd.double().tolist())
        assert abs(sum_squares(xd) - exact) <= 4101 * 2.0 ** -53 * exact
    with pytest.raises(ValueError):
        sum_squares(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        sum_squares([np.zeros(4)])


def test_sum_squares_sequence_equals_concatenation():
    # integer values: every partial sum is exact, so equality is exact
    g = torch.Generator().manual_seed(5)
    parts = [torch.randint(-100, 100, (k,), generator=g).float()
             for k in (1, 17, 300, 0)]
    parts[1] = parts[1].to(torch.bfloat16)
    cat = torch.cat([p.float() for p in parts])
    assert sum_squares(parts) == sum_squares(cat) == float((cat.double() ** 2
                                                            ).sum())
    assert sum_squares(tuple(parts[:1])) == sum_squares(parts[0])
    assert sum_squares([]) == 0.0


def test_clip_factor():
    x = torch.tensor([3.0, 4.0])  # norm 5
    assert clip_factor(x, 10.0) == 1.0  # below the bound
    assert clip_factor(x, 5.0) == 1.0
    assert clip_factor(x, 1.0) == 1.0 / 5.0  # above the bound
    assert clip_factor([x, torch.tensor([12.0])], 6.5) == 0.5  # norm 13
    assert clip_factor(torch.zeros(8), 1.0) == 1.0  # zero vector
    assert clip_factor(torch.zeros(0), 1.0) == 1.0
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            clip_factor(torch.tensor([1.0, bad]), 1.0)
    for bad_norm in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            clip_factor(x, bad_norm)
    # the clipped, weighted update has norm <= weight * clip_norm
    g = torch.Generator().manual_seed(6)
    u = torch.randn(1000, generator=g) * 7
    c = clip_factor(u, 2.0)
    assert math.sqrt(sum_squares(u * c)) <= 2.0 * (1 + 1e-6)
