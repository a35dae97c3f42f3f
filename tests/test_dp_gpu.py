"""GPU tests (MI355X): the differential-privacy kernels — quantise + binomial
noise + masks in one pass, and the float64 sum of squares — against the
numpy specification (rayfed_amd/ops/secagg_ref.py), bit for bit where the
spec is exact.  Single process; every reference stream is computed once at
the largest length and sliced."""
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

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="requires MI355X"
)

NSTRIDE = 2 * 16 * 256 + 17  # one 256-lane block loops 2-3 times over this
NMAX = NSTRIDE
ROUND = (5 << 32) | 0x9ABCDEF1
FRAC = 16
WEIGHT = 0.3
KEYS = [hashlib.sha256(b"dp-gpu-test-%d" % i).digest() for i in range(15)]
SIGNS = [1 if (i * 5 + 1) % 3 else -1 for i in range(15)]  # mixed
NOISE_KEY = hashlib.sha256(b"dp-gpu-noise").digest()
NOISE_PARAMS = [(1, 1), (4, 1000), (16, 1 << 20)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def ext():
    from rayfed_amd.ops import _hip_loader

    return _hip_loader.load()


def _key_tensors(idx):
    kt = torch.from_numpy(
        np.frombuffer(b"".join(KEYS[i] for i in idx), dtype=np.uint8).copy()
    ).reshape(len(idx), 32)
    return kt, torch.tensor([SIGNS[i] for i in idx], dtype=torch.int32)


def _noise_key_tensor(key=NOISE_KEY):
    return torch.from_numpy(np.frombuffer(key, dtype=np.uint8).copy())


@functools.lru_cache(maxsize=None)
def _signed_sum(count):
    """sum_{i<count} SIGNS[i] * KS(KEYS[i], ROUND, e), e < NMAX (uint32)."""
    acc = np.zeros(NMAX, dtype=np.uint32)
    for i in range(count):
        ks = ref.keystream(KEYS[i], ROUND, 0, NMAX)
        if SIGNS[i] > 0:
            acc += ks
        else:
            acc -= ks
    acc.setflags(write=False)
    return acc


@functools.lru_cache(maxsize=None)
def _noise(words, step):
    z = ref.binomial_noise(NOISE_KEY, ROUND, 0, NMAX, words, step)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _update(dtype_name):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(NMAX, generator=g) * 50.0
    x[5] = 40000.0  # saturates
    x[11] = float("nan")
    return x.to(DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def _quantized(dtype_name):
    q = ref.quantize(_update(dtype_name).float().numpy(), WEIGHT,
                     FRAC).view(np.uint32)
    q.setflags(write=False)
    return q


def _want(dtype_name, n, peers, words, step):
    return (_quantized(dtype_name)[:n] + _noise(words, step)[:n]
            + _signed_sum(peers)[:n]).view(np.int32)


# ------------------------------------------------------------ noise kernel
@needs_gpu
@pytest.mark.parametrize("words,step", NOISE_PARAMS)
@pytest.mark.parametrize("peers", [0, 1, 15])
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 4101])
def test_noise_kernel_matches_reference(ext, n, dtype_name, peers, words,
                                        step):
    x = _update(dtype_name)[:n].cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    kt, st = _key_tensors(range(peers))
    ext.secagg_mask_noise_async(x, out, kt, st, _noise_key_tensor(), words,
                                step, ROUND, 0, WEIGHT, FRAC)
    assert np.array_equal(out.cpu().numpy(),
                          _want(dtype_name, n, peers, words, step))


@needs_gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8, 16])
def test_noise_kernel_every_word_count(ext, words):
    n = 4101
    x = _update("bf16")[:n].cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    kt, st = _key_tensors(range(2))
    ext.secagg_mask_noise_async(x, out, kt, st, _noise_key_tensor(), words,
                                77, ROUND, 0, WEIGHT, FRAC)
    assert np.array_equal(out.cpu().numpy(), _want("bf16", n, 2, words, 77))


@needs_gpu
@pytest.mark.parametrize("words,step", NOISE_PARAMS)
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_noise_kernel_grid_stride(ext, dtype_name, words, step):
    n = NSTRIDE
    x = _update(dtype_name)[:n].cuda()
    kt, st = _key_tensors(range(2))
    want = _want(dtype_name, n, 2, words, step)
    for max_blocks in (1, 2):
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        ext.secagg_mask_noise_async(x, out, kt, st, _noise_key_tensor(),
                                    words, step, ROUND, 0, WEIGHT, FRAC,
                                    max_blocks=max_blocks)
        assert np.array_equal(out.cpu().numpy(), want), max_blocks


@needs_gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_noise_kernel_misaligned_views(ext, dtype_name):
    n = 4101
    words, step = 4, 1000
    kt, st = _key_tensors(range(2))
    nk = _noise_key_tensor()
    xhost = _update(dtype_name)[1 : n + 1]
    want = ref.mask_noise_ref(xhost.float().numpy(), WEIGHT, FRAC, KEYS[:2],
                              SIGNS[:2], ROUND, 0, NOISE_KEY, words, step)
    xbuf = _update(dtype_name)[: n + 1].cuda()
    x_mis, x_al = xbuf[1:], xbuf[1:].clone()
    assert x_mis.data_ptr() % 16 != 0 and x_al.data_ptr() % 16 == 0
    for x, out_misaligned in ((x_mis, True), (x_al, True), (x_mis, False)):
        obuf = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
        out = obuf[1:] if out_misaligned else obuf[:n]
        ext.secagg_mask_noise_async(x, out, kt, st, nk, words, step, ROUND,
                                    0, WEIGHT, FRAC)
        assert np.array_equal(out.cpu().numpy(), want)
        guard = obuf[0] if out_misaligned else obuf[n]
        assert int(guard) == 7  # the guard element is untouched


@needs_gpu
@pytest.mark.parametrize("words,offset", [(4, 16), (4, 2 ** 34 - 48),
                                          (16, 2 ** 32 - 48)])
def test_noise_kernel_offsets(ext, words, offset):
    n = 40
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=g)
    kt, st = _key_tensors(range(3))
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    ext.secagg_mask_noise_async(x.cuda(), out, kt, st, _noise_key_tensor(),
                                words, 9, ROUND, offset, 1.0, FRAC)
    want = ref.mask_noise_ref(x.numpy(), 1.0, FRAC, KEYS[:3], SIGNS[:3],
                              ROUND, offset, NOISE_KEY, words, 9)
    assert np.array_equal(out.cpu().numpy(), want)


@needs_gpu
def test_noise_kernel_validation_launches_nothing(ext):
    kt, st = _key_tensors(range(1))
    nk = _noise_key_tensor()
    x = torch.zeros(49, device="cuda")
    out = torch.full((49,), 7, dtype=torch.int32, device="cuda")

    def call(xx=x, oo=out, nkey=nk, words=4, step=1, offset=0, frac=FRAC):
        ext.secagg_mask_noise_async(xx, oo, kt, st, nkey, words, step, ROUND,
                                    offset, 1.0, frac)

    for words, top in ((4, 2 ** 34 - 48), (16, 2 ** 32 - 48)):
        with pytest.raises(RuntimeError):  # one element past the limit
            call(words=words, offset=top)
        call(xx=x[:48], oo=out[:48], words=words, offset=top)  # at the limit
        assert int(out[48]) == 7
        out.fill_(7)
    for bad in (dict(words=3), dict(words=32), dict(step=0),
                dict(step=(1 << 20) + 1), dict(offset=8), dict(frac=31),
                dict(nkey=nk[:31].clone()), dict(nkey=nk.cuda()),
                dict(oo=out.cpu())):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((out == 7).all())  # nothing was launched
    s = SecAggSession(["a", "b"], "a", {"b": KEYS[0]})
    with pytest.raises(ValueError):
        s.mask(x, round=ROUND, offset=2 ** 34 - 48,
               noise=BinomialNoise(NOISE_KEY, words=4))


# ---------------------------------------------------------- sum of squares
def _sumsq_input(dtype_name):
    g = torch.Generator().manual_seed(9)
    x = torch.randn((1 << 20) + 4, generator=g) * 3.0
    return x.to(DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def _sumsq_dev(dtype_name):
    return _sumsq_input(dtype_name).cuda()


@needs_gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n", [0, 1, 255, 4101, (1 << 20) + 3])
def test_sumsq_matches_reference(ext, n, dtype_name):
    """Squares are exact in double; a sum of n non-negative doubles in any
    order is within (n-1)*2^-53 of the true sum, relative — for the kernel
    and for numpy — so the two agree within n*2^-52."""
    xd = _sumsq_dev(dtype_name)
    for lo in (0, 1):  # aligned, and a misaligned view of the same length
        x = xd[lo : lo + n]
        got = ext.sumsq_async(x)
        assert got.dtype == torch.float64 and got.shape == (1,)
        assert got.device == x.device
        want = ref.sum_squares_ref(x.cpu().float().numpy())
        assert abs(got.item() - want) <= n * 2.0 ** -52 * want
        if n == 0:
            assert got.item() == 0.0
        else:
            assert got.item() > 0.0
        assert sum_squares(x) == got.item()


@needs_gpu
def test_sumsq_large_values_nonfinite_and_reproducible(ext):
    for dt in (torch.float32, torch.bfloat16):
        x = torch.full((4101,), 1e30, dtype=dt, device="cuda")
        v = float(x[0].double()) ** 2
        got = ext.sumsq_async(x).item()
        assert math.isfinite(got)
        assert abs(got - 4101 * v) <= 4101 * 2.0 ** -52 * 4101 * v
    base = _sumsq_dev("fp32")[:4101].clone()
    for bad in (float("inf"), float("-inf"), float("nan")):
        for pos in (0, 4100, 2000):
            x = base.clone()
            x[pos] = bad
            got = ext.sumsq_async(x).item()
            assert math.isnan(got) if bad != bad else got == math.inf
            with pytest.raises(ValueError):
                clip_factor(x, 1.0)
    x = _sumsq_dev("bf16")[: (1 << 20) + 3]
    a, b = ext.sumsq_async(x), ext.sumsq_async(x)
    assert a.cpu().view(torch.int64).item() == b.cpu().view(torch.int64).item()
    with pytest.raises(RuntimeError):
        ext.sumsq_async(torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        ext.sumsq_async(torch.zeros(4))


@needs_gpu
def test_sum_squares_and_clip_factor_on_device():
    xd = _sumsq_dev("fp32")
    parts = [xd[:4096], xd[4096:4101].to(torch.bfloat16), xd[8192:8192 + 255]]
    want = sum(ref.sum_squares_ref(p.cpu().float().numpy()) for p in parts)
    n = sum(p.numel() for p in parts)
    got = sum_squares(parts)
    assert abs(got - want) <= n * 2.0 ** -52 * want
    # a CPU tensor in the sequence is summed by the reference
    mixed = sum_squares([parts[0], parts[1].cpu(), parts[2]])
    assert abs(mixed - want) <= n * 2.0 ** -52 * want
    norm = math.sqrt(want)
    assert clip_factor(parts, 2 * norm) == 1.0
    c = clip_factor(parts, norm / 4)
    assert c == pytest.approx(0.25, rel=1e-12)
    assert clip_factor(torch.zeros(100, device="cuda"), 1.0) == 1.0
    with pytest.raises(ValueError):
        sum_squares(xd[::2])  # not contiguous


# --------------------------------------------------------------- public API
@needs_gpu
def test_five_party_dp_round_with_dropout_matches_cpu():
    parties = ["alice", "bob", "carol", "dave", "erin"]
    dropped = ["bob", "erin"]
    survivors = [p for p in parties if p not in dropped]
    n = 4101
    clip = 30.0
    sess = {p: SecAggSession.from_shared_secret(parties, p, b"dp-gpu-round")
            for p in parties}
    noises = {p: BinomialNoise(hashlib.sha256(b"nz" + p.encode()).digest(),
                               words=4, step=50) for p in parties}
    ups = {}
    for i, p in enumerate(parties):
        g = torch.Generator().manual_seed(40 + i)
        ups[p] = (torch.randn(n, generator=g) * (0.2 * (i + 1))
                  ).to(torch.bfloat16)
    # the norm on either device agrees within the summation-order bound;
    # one set of weights (from the device norm) then drives both paths
    w = {}
    for i, p in enumerate(parties):
        c_dev = clip_factor(ups[p].cuda(), clip)
        c_cpu = clip_factor(ups[p], clip)
        assert abs(c_dev - c_cpu) <= n * 2.0 ** -52 * c_cpu
        w[p] = 0.125 * (i + 1) * c_dev
    assert any(clip_factor(ups[p], clip) < 1.0 for p in survivors)
    assert any(clip_factor(ups[p], clip) == 1.0 for p in survivors)
    revealed = {p: sess[p].reveal(dropped) for p in survivors}

    def run(device, out_dtype):
        masked = {p: sess[p].mask(ups[p].to(device), round=21, weight=w[p],
                                  noise=noises[p])
                  for p in survivors}
        out = aggregate(masked, parties, round=21, out_dtype=out_dtype,
                        revealed=revealed)
        return {p: m.cpu() for p, m in masked.items()}, out.cpu()

    for out_dtype in (torch.float32, torch.bfloat16):
        m_cpu, o_cpu = run("cpu", out_dtype)
        m_gpu, o_gpu = run("cuda", out_dtype)
        for p in survivors:
            assert torch.equal(m_cpu[p], m_gpu[p])
        assert o_gpu.dtype == out_dtype and torch.equal(o_cpu, o_gpu)
    # and the result is the survivors' quantised sum plus their noises
    acc = np.zeros(n, dtype=np.uint32)
    for p in survivors:
        acc += ref.quantize(ups[p].float().numpy(), w[p], 16).view(np.uint32)
        acc += ref.binomial_noise(noises[p].key, 21, 0, n, 4, 50)
    _, o32 = run("cuda", torch.float32)
    assert np.array_equal(o32.numpy(),
                          acc.view(np.int32).astype(np.float32)
                          * np.float32(2.0 ** -16))


@needs_gpu
def test_noise_none_on_device_is_the_plain_mask():
    n = 4101
    s = SecAggSession(["a", "b", "c"], "b", {"a": KEYS[0], "c": KEYS[1]})
    x = _update("bf16")[:n]
    want = ref.mask_ref(x.float().numpy(), WEIGHT, FRAC, KEYS[:2], [-1, 1],
                        ROUND, 16)
    got = s.mask(x.cuda(), round=ROUND, weight=WEIGHT, offset=16, noise=None)
    assert np.array_equal(got.cpu().numpy(), want)
    got = s.mask(x.cuda(), round=ROUND, weight=WEIGHT, offset=16)
    assert np.array_equal(got.cpu().numpy(), want)


@needs_gpu
def test_mixed_devices_rejected_with_noise():
    s = SecAggSession(["a", "b"], "a", {"b": KEYS[0]})
    noise = BinomialNoise(NOISE_KEY)
    with pytest.raises(ValueError):
        s.mask(torch.zeros(40, device="cuda"), round=0, noise=noise,
               out=torch.zeros(40, dtype=torch.int32))
    with pytest.raises(ValueError):
        s.mask(torch.zeros(40), round=0, noise=noise,
               out=torch.zeros(40, dtype=torch.int32, device="cuda"))
