"""GPU tests (MI355X): the secure-aggregation HIP kernels against the numpy
reference, bit for bit.  Single process; every reference keystream is
computed once at the largest length and sliced."""
import functools
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from rayfed_amd.ops import secagg_ref as ref  # noqa: E402
from rayfed_amd.parallel import SecAggSession, aggregate  # noqa: E402

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="requires MI355X"
)

NMAX = (1 << 20) + 3
NPAD = (1 << 20) + 16  # row stride that keeps every row 16-byte aligned
ROUND = (5 << 32) | 0x9ABCDEF1
FRAC = 16
WEIGHT = 0.3
KEYS = [hashlib.sha256(b"secagg-gpu-test-%d" % i).digest() for i in range(64)]
SIGNS = [1 if (i * 5 + 1) % 3 else -1 for i in range(64)]  # mixed
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


@functools.lru_cache(maxsize=None)
def _signed_sum(count):
    """sum_{i<count} SIGNS[i] * KS(KEYS[i], ROUND, e), e < NMAX (uint32)."""
    if count == 0:
        return np.zeros(NMAX, dtype=np.uint32)
    lo = max(c for c in (0, 1, 2, 15) if c < count)  # build on a cached sum
    acc = _signed_sum(lo).copy()
    for i in range(lo, count):
        ks = ref.keystream(KEYS[i], ROUND, 0, NMAX)
        if SIGNS[i] > 0:
            acc += ks
        else:
            acc -= ks
    return acc


@functools.lru_cache(maxsize=None)
def _update(dtype_name):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(NMAX, generator=g) * 50.0
    x[5] = 40000.0  # saturates
    x[11] = float("nan")
    return x.to(DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def _quantized(dtype_name):
    return ref.quantize(_update(dtype_name).float().numpy(), WEIGHT,
                        FRAC).view(np.uint32)


# ------------------------------------------------------------- mask kernel
@needs_gpu
@pytest.mark.parametrize("peers", [1, 2, 15])
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 4101, NMAX])
def test_mask_kernel_matches_reference(ext, n, dtype_name, peers):
    x = _update(dtype_name)[:n].cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    kt, st = _key_tensors(range(peers))
    ext.secagg_mask_async(x, out, kt, st, ROUND, 0, WEIGHT, FRAC)
    want = (_quantized(dtype_name)[:n] + _signed_sum(peers)[:n]).view(np.int32)
    assert np.array_equal(out.cpu().numpy(), want)


@needs_gpu
@pytest.mark.parametrize("offset", [16, (2 ** 32 - 3) * 16])
def test_mask_offsets(ext, offset):
    n = 40
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=g)
    kt, st = _key_tensors(range(3))
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    ext.secagg_mask_async(x.cuda(), out, kt, st, ROUND, offset, 1.0, FRAC)
    want = ref.mask_ref(x.numpy(), 1.0, FRAC, KEYS[:3], SIGNS[:3], ROUND,
                        offset)
    assert np.array_equal(out.cpu().numpy(), want)


@needs_gpu
def test_mask_counter_limit_raises(ext):
    n = 40
    x = torch.zeros(n, device="cuda")
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    kt, st = _key_tensors(range(1))
    bad = (2 ** 32 - 2) * 16
    with pytest.raises(RuntimeError):
        ext.secagg_mask_async(x, out, kt, st, ROUND, bad, 1.0, FRAC)
    with pytest.raises(RuntimeError):
        ext.secagg_mask_async(x, out, kt, st, ROUND, 8, 1.0, FRAC)
    with pytest.raises(RuntimeError):
        ext.secagg_mask_async(x, out, kt, st, ROUND, 0, 1.0, 31)
    s = SecAggSession(["a", "b"], "a", {"b": KEYS[0]})
    with pytest.raises(ValueError):
        s.mask(x, round=ROUND, offset=bad)


@needs_gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_mask_misaligned_views_and_out(dtype_name):
    n = 4101
    s = SecAggSession(["a", "b", "c"], "b", {"a": KEYS[0], "c": KEYS[1]})
    x = _update(dtype_name)[: n + 1]
    want = s.mask(x[1:], round=ROUND, weight=WEIGHT)  # CPU reference path
    xbuf = x.cuda()
    obuf = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    got = s.mask(xbuf[1:], round=ROUND, weight=WEIGHT, out=obuf[1:])
    assert got.data_ptr() == obuf[1:].data_ptr()
    assert int(obuf[0]) == 0
    assert torch.equal(obuf[1:].cpu(), want)
    # aligned input, misaligned output and the other way round
    got = s.mask(xbuf[1:].clone(), round=ROUND, weight=WEIGHT, out=obuf[1:])
    assert torch.equal(got.cpu(), want)
    got = s.mask(xbuf[1:], round=ROUND, weight=WEIGHT)
    assert torch.equal(got.cpu(), want)


S = 2.0 ** -16
EDGES = [0.5 * S, 1.5 * S, 2.5 * S, 0.1, 32767.99, 40000.0, -40000.0,
         float("inf"), float("-inf"), float("nan")]
EDGE_WANT = [0, 2, 2, 6554, 2147483008, 2 ** 31 - 1, -(2 ** 31),
             2 ** 31 - 1, -(2 ** 31), 0]


@needs_gpu
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
def test_quantize_edges_through_kernel(ext, dtype_name):
    dt = DTYPES[dtype_name]
    x32 = torch.tensor(EDGES, dtype=torch.float32)
    x = x32.to(dt)
    # keep the cases this dtype represents exactly (NaN always)
    keep = [i for i in range(len(EDGES))
            if EDGES[i] != EDGES[i] or float(x[i]) == float(x32[i])]
    assert len(keep) >= 5
    # no peers: the kernel output is the quantised value itself
    kt, st = _key_tensors([])
    for xs in (x, torch.cat([x, x])):  # ragged scalar path and vector path
        out = torch.empty(xs.numel(), dtype=torch.int32, device="cuda")
        ext.secagg_mask_async(xs.cuda(), out, kt, st, 0, 0, 1.0, FRAC)
        got = out.cpu().tolist()
        assert got == ref.quantize(xs.float().numpy(), 1.0, FRAC).tolist()
        for i in keep:
            assert got[i] == EDGE_WANT[i], (EDGES[i], got[i])
    # weight path: fl32(x * 0.25) then the exact scale
    xw = torch.tensor([6 * S, 10 * S, 0.4, -160000.0] * 4)
    out = torch.empty(16, dtype=torch.int32, device="cuda")
    ext.secagg_mask_async(xw.cuda(), out, kt, st, 0, 0, 0.25, FRAC)
    assert out.cpu().tolist() == ref.quantize(xw.numpy(), 0.25,
                                              FRAC).tolist()
    assert out.cpu().tolist()[:2] == [2, 2]


# -------------------------------------------------------- aggregate kernel
@pytest.fixture(scope="module")
def agg_inputs():
    rng = np.random.default_rng(11)
    host = rng.integers(-(2 ** 31), 2 ** 31, size=(16, NPAD), dtype=np.int64
                        ).astype(np.int32)
    dev = torch.from_numpy(host).cuda()
    sums = {}
    acc = np.zeros(NPAD, dtype=np.uint32)
    for k in range(16):
        acc = acc + host[k].view(np.uint32)
        if k + 1 in (1, 2, 16):
            sums[k + 1] = acc[:NMAX].copy()
    return dev, sums


@needs_gpu
@pytest.mark.parametrize("out_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [0, 1, 64])
@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("n", [1, 17, 4101, NMAX])
def test_aggregate_kernel_matches_reference(ext, agg_inputs, n, K, C,
                                            out_name):
    dev, sums = agg_inputs
    dt = DTYPES[out_name]
    out = torch.empty(n, dtype=dt, device="cuda")
    kt, st = _key_tensors(range(C))
    ext.secagg_aggregate_async(out, [dev[k, :n] for k in range(K)], kt, st,
                               ROUND, 0, FRAC)
    s = (sums[K][:n] - _signed_sum(C)[:n]).view(np.int32)
    f = s.astype(np.float32) * np.float32(S)
    want = ref.cast_ref(f, {"fp32": "float32", "bf16": "bfloat16",
                            "fp16": "float16"}[out_name])
    got = out.cpu()
    if out_name == "bf16":
        got = got.view(torch.int16)
        want = want.view(np.int16)
    assert np.array_equal(got.numpy(), want)


@needs_gpu
def test_aggregate_misaligned_and_offset(ext, agg_inputs):
    dev, _ = agg_inputs
    n = 4101
    ins = [dev[k, 1 : n + 1] for k in range(3)]
    obuf = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    kt, st = _key_tensors(range(2))
    off = 4096
    ext.secagg_aggregate_async(obuf[1:], ins, kt, st, ROUND, off, FRAC)
    want = ref.aggregate_ref([t.cpu().numpy() for t in ins], KEYS[:2],
                             SIGNS[:2], ROUND, off, FRAC)
    assert float(obuf[0]) == 0.0
    assert np.array_equal(obuf[1:].cpu().numpy(), want)


# --------------------------------------------------------------- public API
@needs_gpu
def test_five_party_round_with_dropout_matches_cpu():
    parties = ["alice", "bob", "carol", "dave", "erin"]
    dropped = ["bob", "erin"]
    survivors = [p for p in parties if p not in dropped]
    n = 4101
    sess = {p: SecAggSession.from_shared_secret(parties, p, b"gpu-round")
            for p in parties}
    ups = {}
    for i, p in enumerate(parties):
        g = torch.Generator().manual_seed(40 + i)
        ups[p] = torch.randn(n, generator=g).to(torch.bfloat16)
    w = {p: 0.125 * (i + 1) for i, p in enumerate(parties)}
    revealed = {p: sess[p].reveal(dropped) for p in survivors}

    def run(device, out_dtype):
        masked = {p: sess[p].mask(ups[p].to(device), round=21, weight=w[p])
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
    # and the result is the survivors' quantised sum
    acc = np.zeros(n, dtype=np.uint32)
    for p in survivors:
        acc += ref.quantize(ups[p].float().numpy(), w[p], 16).view(np.uint32)
    _, o32 = run("cuda", torch.float32)
    assert np.array_equal(o32.numpy(),
                          acc.view(np.int32).astype(np.float32)
                          * np.float32(S))


@needs_gpu
def test_mixed_devices_rejected():
    a = torch.zeros(40, dtype=torch.int32)
    with pytest.raises(ValueError):
        aggregate({"a": a, "b": a.cuda()}, ["a", "b"], round=0)
    s = SecAggSession(["a", "b"], "a", {"b": KEYS[0]})
    with pytest.raises(ValueError):
        s.mask(torch.zeros(40, device="cuda"), round=0,
               out=torch.zeros(40, dtype=torch.int32))
