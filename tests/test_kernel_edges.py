"""GPU tests (MI355X): the data-plane kernels of csrc/rayfed_hip.hip against
exact CPU references at their edges.

References: rayfed_amd/ops/fp8_ref.py (fp8 wire), rayfed_amd/ops/hash_ref.py
(hash64), zlib (CRC32) and float64 numpy sums (weighted reduce).  Every
tolerance below is derived from the number formats, never from kernel output.
Inputs and references are built on the CPU once per module and shared.
"""
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from rayfed_amd.ops import fp8_ref  # noqa: E402
from rayfed_amd.ops.hash_ref import hash64_ref  # noqa: E402

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="requires MI355X"
)

M64 = 0xFFFFFFFFFFFFFFFF
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
VEC = {"bf16": 8, "fp16": 8, "fp32": 4}  # elements per 16-byte lane access
PBITS = {"bf16": 8, "fp16": 11, "fp32": 24}  # significand bits
EMIN = {"bf16": -126, "fp16": -14, "fp32": -126}  # smallest normal exponent
GRID = 4096 * 256  # lanes of one grid-stride sweep (reduce / masked_add)
HASH_W = 8 * 4 * 524288  # bytes covered by one hash64 slot sweep (16 MiB)


@pytest.fixture(scope="module")
def ext():
    from rayfed_amd.ops import _hip_loader

    return _hip_loader.load()


# ------------------------------------------------------------------ helpers
def _bits(t):
    """Integer view of a float tensor (bit-exact comparisons, NaN-safe)."""
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _f64(t):
    return t.detach().cpu().double().numpy()


def _bf16_from_bits(bits_u16):
    return torch.from_numpy(
        np.asarray(bits_u16, dtype=np.uint16).view(np.int16).copy()
    ).view(torch.bfloat16)


def _bf16_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _ulp(v, name):
    """Spacing of the format at magnitude |v| (subnormal spacing below 2^EMIN)."""
    _, e = np.frexp(np.abs(v))  # |v| = m * 2^e, m in [0.5, 1)
    e = np.maximum(e - 1, EMIN[name])
    return np.ldexp(1.0, e - (PBITS[name] - 1))


def _rne(x, name):
    """float64 -> nearest value of the format, ties to even (normal range)."""
    m, e = np.frexp(x)
    return np.ldexp(np.rint(np.ldexp(m, PBITS[name])), e - PBITS[name])


def _f32_to_bf16_bits(f32):
    """IEEE float32 array -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def _check_weighted_sum(out, ins, w_used, name, factor=None):
    """|out - ref| <= 0.5 ulp(max(|ref|,|out|)) + factor * S  per element.

    ref = sum float64(w_i) * float64(x_i),  S = sum |w_i x_i|.  The first
    term is the one permitted rounding to the output format.  The default
    factor (k+1) * 2^-23 bounds k fp32 multiply-adds, fused or not, plus the
    double->float rounding of the weights.  Non-finite reference elements
    must match in kind and sign.  Returns the largest |out-ref| beyond the
    half-ulp term in units of S (for reporting).
    """
    k = len(ins)
    if factor is None:
        factor = (k + 1) * 2.0 ** -23
    xs = [_f64(x) for x in ins]
    with np.errstate(invalid="ignore", over="ignore"):
        ref = sum(w * x for w, x in zip(w_used, xs))
        S = sum(np.abs(w * x) for w, x in zip(w_used, xs))
    o = _f64(out)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(o), np.isnan(ref)), "NaN positions differ"
    assert np.array_equal(np.isinf(o), np.isinf(ref)), "Inf positions differ"
    inf = np.isinf(ref)
    assert np.array_equal(np.signbit(o[inf]), np.signbit(ref[inf]))
    o, ref, S = o[fin], ref[fin], S[fin]
    err = np.abs(o - ref)
    half = 0.5 * _ulp(np.maximum(np.abs(ref), np.abs(o)), name)
    bad = np.flatnonzero(err > half + factor * S)
    assert bad.size == 0, (
        f"{bad.size} elements out of bound; first at {bad[0]}: out={o[bad[0]]!r} "
        f"ref={ref[bad[0]]!r} S={S[bad[0]]!r}"
    )
    with np.errstate(invalid="ignore", divide="ignore"):
        excess = np.where(S > 0, (err - half) / S, 0.0)
    return float(excess.max()) if excess.size else 0.0


@functools.lru_cache(maxsize=None)
def _scaled_inputs(name, n, k):
    """k CPU tensors of randn * 2^e with one exponent e per element, so small
    magnitudes are held to the same relative bound as large ones.  fp16 can
    not hold 2^20 (max 65504): its exponents stop at 2^11."""
    g = torch.Generator().manual_seed(1000 * n % 99991 + 31 * k + len(name))
    hi = 11 if name == "fp16" else 20
    e = torch.randint(-20, hi + 1, (n,), generator=g)
    scale = torch.ldexp(torch.ones(n), e)
    return tuple(
        (torch.randn(n, generator=g) * scale).to(DTYPES[name]) for _ in range(k)
    )


def _weights(k):
    """Not dyadic, so rounding them to bf16 or truncating would show."""
    if k <= 2:
        return [0.3, 0.7][:k]
    return [(i + 1) / (k * (k + 1) / 2) for i in range(k)]


def _w32(w):
    return [float(np.float32(x)) for x in w]


def _wbf16(w):
    b = _f32_to_bf16_bits(np.asarray(w, dtype=np.float32))
    return [float(v) for v in _bf16_from_bits(b).double().numpy()]


@functools.lru_cache(maxsize=None)
def _fp8_encode_lut():
    """fp8 byte of every bf16 bit pattern, by the CPU reference."""
    x = _bf16_from_bits(np.arange(65536, dtype=np.uint16)).double().numpy()
    return fp8_ref.encode(x)


@functools.lru_cache(maxsize=None)
def _fp8_decode_lut():
    """(bf16 bits of every decoded byte, NaN mask).  Decodes are exact in bf16."""
    d = fp8_ref.decode(np.arange(256, dtype=np.uint8))
    nan = np.isnan(d)
    bits = _bf16_bits(torch.from_numpy(np.where(nan, 0.0, d)).to(torch.bfloat16))
    return bits, nan


def _pattern_bits(n):
    """bf16 bit patterns: a fixed permutation of all 65,536, repeated."""
    return ((np.arange(n, dtype=np.uint64) * 40503 + 12345) & 0xFFFF).astype(np.uint16)


SENT = 0xA5  # sentinel byte past the end of outputs


# ------------------------------------------------------------------ fp8 pack
def _run_pack(ext, which, src_bits):
    """Pack a bf16 buffer; assert bytes == reference, checksum, sentinel."""
    n = len(src_bits)
    src = _bf16_from_bits(src_bits).cuda()
    dst = torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda")
    fn = {"crc": ext.pack_fp8_async, "hash": ext.pack_fp8_hash64_async}[which]
    ck = fn(src, dst)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    want = _fp8_encode_lut()[src_bits]
    bad = np.flatnonzero(got[:n] != want)
    assert bad.size == 0, (
        f"{bad.size} fp8 bytes differ; first at {bad[0]}: bf16 "
        f"{src_bits[bad[0]]:#06x} -> {got[bad[0]]:#04x}, want {want[bad[0]]:#04x}"
    )
    assert (got[n:] == SENT).all(), "wrote past n"
    if which == "crc":
        assert (int(ck[2].item()) & 0xFFFFFFFF) == zlib.crc32(want.tobytes())
    else:
        assert (int(ck.item()) & M64) == hash64_ref(want.tobytes())
    return got[:n]


@needs_gpu
@pytest.mark.parametrize("which", ["crc", "hash"])
def test_pack_fp8_every_bf16_pattern(ext, which):
    _run_pack(ext, which, np.arange(65536, dtype=np.uint16))


# (value, hand-derived byte).  Ties go to the even mantissa; |x| < 2^-6 is the
# subnormal range (multiples of 2^-9); finite values above 448 saturate;
# non-finite values become the NaN byte with the sign kept.
FP8_EDGES = [
    (2.0 ** -10, 0x00), (-(2.0 ** -10), 0x80), (3 * 2.0 ** -10, 0x02),
    (5 * 2.0 ** -10, 0x02), (15 * 2.0 ** -10, 0x08), (1.0625, 0x38),
    (1.1875, 0x3A),
    (2.0 ** -9, 0x01), (7 * 2.0 ** -9, 0x07), (-3 * 2.0 ** -9, 0x83),
    (2.0 ** -20, 0x00), (2.0 ** -6, 0x08), (0.0, 0x00), (-0.0, 0x80),
    (448.0, 0x7E), (-448.0, 0xFE), (464.0, 0x7E), (3e38, 0x7E), (-3e38, 0xFE),
    (float("inf"), 0x7F), (float("-inf"), 0xFF),
    (float("nan"), 0x7F), (480.0, 0x7E), (432.0, 0x7E), (400.0, 0x7C),
    (-1.0, 0xB8), (0.5, 0x30), (-432.0, 0xFE),
]


@needs_gpu
@pytest.mark.parametrize("which", ["crc", "hash"])
@pytest.mark.parametrize("chunk", range(len(FP8_EDGES) // 7))
def test_pack_fp8_edges_in_scalar_tail(ext, which, chunk):
    """n = 4096 + 7: the last 7 elements take the scalar tail loop."""
    edges = FP8_EDGES[7 * chunk : 7 * chunk + 7]
    vals = torch.tensor([v for v, _ in edges], dtype=torch.float64)
    bits = _pattern_bits(4096 + 7)
    bits[4096:] = _bf16_bits(vals.to(torch.bfloat16))
    got = _run_pack(ext, which, bits)
    assert got[4096:].tolist() == [b for _, b in edges]


@needs_gpu
def test_pack_fp8_negative_nan_keeps_sign(ext):
    bits = _pattern_bits(4096 + 7)
    bits[5] = 0xFFC0  # vector body
    bits[4096 + 2] = 0xFFFF  # tail
    for which in ("crc", "hash"):
        got = _run_pack(ext, which, bits)
        assert got[5] == 0xFF and got[4096 + 2] == 0xFF


@needs_gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4095, 4096, 4097, 4096 * 256 + 9])
def test_pack_fp8_sizes(ext, n):
    _run_pack(ext, "crc", _pattern_bits(n))


HASH_FP8_SIZES = [0, 1, 7, 8, 9, 31, 32, 33, 16_777_216 + 43]


@needs_gpu
@pytest.mark.parametrize("n", HASH_FP8_SIZES)
def test_pack_fp8_hash64_sizes(ext, n):
    """The last size is a second slot sweep with a partial group and a tail."""
    _run_pack(ext, "hash", _pattern_bits(n))


@needs_gpu
@pytest.mark.parametrize("off", [1, 3])
def test_pack_fp8_misaligned_views(ext, off):
    """Views at odd element offsets are rerouted to the scalar path; the
    hash64 variant rejects them."""
    n = 4096 + 9
    bits = _pattern_bits(n + 8)
    src = _bf16_from_bits(bits).cuda()[off : off + n]
    want = _fp8_encode_lut()[bits[off : off + n]]
    for doff in (0, off):
        buf = torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda")
        ck = ext.pack_fp8_async(src, buf[doff : doff + n])
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[doff : doff + n], want)
        assert (got[:doff] == SENT).all() and (got[doff + n :] == SENT).all()
        assert (int(ck[2].item()) & 0xFFFFFFFF) == zlib.crc32(want.tobytes())
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        ext.pack_fp8_hash64_async(src, dst)


# ---------------------------------------------------------------- fp8 unpack
def _run_unpack(ext, which, src_bytes, src_dev=None, guard=8):
    """Expand fp8 bytes; assert bf16 bits == reference, NaN via isnan, guards."""
    n = len(src_bytes)
    src = torch.from_numpy(src_bytes).cuda() if src_dev is None else src_dev
    buf = torch.full((n + 2 * guard,), 0x1234, dtype=torch.int16, device="cuda")
    dst = buf[guard : guard + n].view(torch.bfloat16)
    if which == "plain":
        ext.unpack_fp8_async(src, dst)
    else:
        hv = ext.unpack_fp8_hash64_async(src, dst)
    torch.cuda.synchronize()
    all_bits = buf.cpu().numpy().view(np.uint16)
    got = all_bits[guard : guard + n]
    lut, nan_lut = _fp8_decode_lut()
    nan = nan_lut[src_bytes]
    bad = np.flatnonzero((got != lut[src_bytes]) & ~nan)
    assert bad.size == 0, (
        f"{bad.size} decodes differ; first at {bad[0]}: byte "
        f"{src_bytes[bad[0]]:#04x} -> {got[bad[0]]:#06x}"
    )
    # NaN: exponent all ones and a non-zero mantissa, whatever the payload.
    is_nan = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
    assert np.array_equal(is_nan, nan), "NaN bytes must decode to NaN"
    assert (all_bits[:guard] == 0x1234).all(), "wrote before dst"
    assert (all_bits[guard + n :] == 0x1234).all(), "wrote past dst"
    if which == "hash":
        assert (int(hv.item()) & M64) == hash64_ref(src_bytes.tobytes())


@needs_gpu
@pytest.mark.parametrize("which", ["plain", "hash"])
def test_unpack_fp8_every_byte_in_body_and_tail(ext, which):
    """37 calls of n = 16 + 7: over the calls every byte value (0x7F, 0xFF and
    0x80 included) lands in the vector body and in the 7-element tail."""
    seen_body, seen_tail = set(), set()
    for r in range(37):
        body = (16 * r + np.arange(16)) % 256
        tail = (7 * r + np.arange(7)) % 256
        seen_body.update(body.tolist())
        seen_tail.update(tail.tolist())
        _run_unpack(ext, which, np.concatenate([body, tail]).astype(np.uint8))
    assert len(seen_body) == 256 and len(seen_tail) == 256


def _byte_pattern(n):
    return ((np.arange(n, dtype=np.uint64) * 167 + 13) & 0xFF).astype(np.uint8)


@needs_gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 256, 8_388_608 + 9])
def test_unpack_fp8_sizes(ext, n):
    """The last size crosses the grid stride of 4096*256*8 elements."""
    _run_unpack(ext, "plain", _byte_pattern(n))


@needs_gpu
@pytest.mark.parametrize("n", HASH_FP8_SIZES)
def test_unpack_fp8_hash64_sizes(ext, n):
    _run_unpack(ext, "hash", _byte_pattern(n))


@needs_gpu
@pytest.mark.parametrize("off", [1, 3])
def test_unpack_fp8_misaligned_views(ext, off):
    n = 256 + 9
    data = _byte_pattern(n + 8)
    src = torch.from_numpy(data).cuda()[off : off + n]
    _run_unpack(ext, "plain", data[off : off + n], src_dev=src)  # src alone
    _run_unpack(ext, "plain", data[:n], guard=off)  # dst alone
    _run_unpack(ext, "plain", data[off : off + n], src_dev=src, guard=off)
    dst = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ext.unpack_fp8_hash64_async(src, dst)


# ------------------------------------------------------------ weighted reduce
def _reduce(ext, name, ins_cpu, w, mfma=False):
    ins = [x.cuda() for x in ins_cpu]
    out = torch.empty_like(ins[0])
    (ext.fedavg_reduce_mfma_ if mfma else ext.fedavg_reduce_)(out, ins, w)
    torch.cuda.synchronize()
    return out.cpu()


def _small_sizes(name):
    v = VEC[name]
    return [1, v - 1, v, v + 1, 2 * v + 3]


@needs_gpu
@pytest.mark.parametrize("k", [1, 2, 16])
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_fedavg_reduce_half_ulp_small(ext, name, k):
    for n in _small_sizes(name):
        ins = _scaled_inputs(name, n, k)
        w = _weights(k)
        out = _reduce(ext, name, ins, w)
        _check_weighted_sum(out, ins, _w32(w), name)


@needs_gpu
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_fedavg_reduce_half_ulp_second_sweep(ext, name):
    """n = 4096*256*VEC + VEC + 1: a second grid-stride sweep plus a tail."""
    n = GRID * VEC[name] + VEC[name] + 1
    ins = _scaled_inputs(name, n, 2)
    w = _weights(2)
    out = _reduce(ext, name, ins, w)
    _check_weighted_sum(out, ins, _w32(w), name)


@needs_gpu
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_fedavg_reduce_ties_to_even(ext, name):
    """Power-of-two weights and inputs chosen so every fp32 step is exact and
    the sum lands on (or just off) a tie of the output format.  With
    u = 2^-(p-1), the spacing at 1:  0.5*1 + 0.5*(1+u) = 1 + u/2 -> 1 (even);
    0.5*(1+u) + 0.5*(1+2u) = 1 + 3u/2 -> 1 + 2u (even)."""
    u = 2.0 ** -(PBITS[name] - 1)
    #        x0        x1        w0    w1    expected
    cases = [
        (1.0, 1 + u, 0.5, 0.5, 1.0),
        (1 + u, 1 + 2 * u, 0.5, 0.5, 1 + 2 * u),
        (-1.0, -(1 + u), 0.5, 0.5, -1.0),
        (-(1 + u), -(1 + 2 * u), 0.5, 0.5, -(1 + 2 * u)),
        (1.0, 1 + u, 0.25, 0.75, 1 + u),  # 1 + 3u/4: above the tie
        (1.0, 1 + u, 0.75, 0.25, 1.0),  # 1 + u/4: below the tie
        (2.0, 2 + 2 * u, 0.5, 0.5, 2.0),  # next binade
        (1 + 6 * u, 1 + 7 * u, 0.5, 0.5, 1 + 6 * u),
    ]
    # Subnormal outputs (fp32 subnormals on the way for bf16): with m the
    # smallest subnormal, (m + 2m)/2 = 1.5m -> 2m and (2m + 3m)/2 -> 2m.
    m = 2.0 ** (EMIN[name] - (PBITS[name] - 1))
    cases += [
        (m, 2 * m, 0.5, 0.5, 2 * m),
        (2 * m, 3 * m, 0.5, 0.5, 2 * m),
        (-m, -2 * m, 0.5, 0.5, -2 * m),
        (m, m, 0.5, 0.5, m),
    ]
    n = 2 * VEC[name] + 3  # vector body and tail both see every case
    dt = DTYPES[name]
    for x0, x1, w0, w1, want in cases:
        a = torch.full((n,), x0, dtype=torch.float64).to(dt)
        b = torch.full((n,), x1, dtype=torch.float64).to(dt)
        assert a.double()[0].item() == x0 and b.double()[0].item() == x1
        out = _reduce(ext, name, [a, b], [w0, w1])
        exp = torch.full((n,), want, dtype=torch.float64).to(dt)
        assert exp.double()[0].item() == want
        if abs(want) >= 2.0 ** EMIN[name]:  # _rne covers the normal range
            assert _rne(np.array([w0 * x0 + w1 * x1]), name)[0] == want
        assert torch.equal(_bits(out), _bits(exp)), (x0, x1, w0, w1, out[0].item())


@needs_gpu
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_fedavg_reduce_exact_grid(ext, name):
    """Inputs on a 2^-6 grid below 4 and dyadic weights: every fp32 product
    and sum is exact, so the output must equal rne(float64 sum) bit for bit
    (ties occur throughout for bf16)."""
    n = 4096 + VEC[name] + 1
    g = torch.Generator().manual_seed(5)
    ins = [
        (torch.randint(-255, 256, (n,), generator=g).double() / 64).to(DTYPES[name])
        for _ in range(4)
    ]
    w = [0.25, 0.5, 0.125, 0.125]
    out = _reduce(ext, name, ins, w)
    ref = sum(wi * _f64(x) for wi, x in zip(w, ins))
    exp = torch.from_numpy(_rne(ref, name)).to(DTYPES[name])
    assert torch.equal(_bits(out), _bits(exp))
    # k = 1, weight 1: the identity.
    out1 = _reduce(ext, name, ins[:1], [1.0])
    assert torch.equal(_bits(out1), _bits(ins[0]))


def _nonfinite_inputs(name, n, rot):
    """Element j carries case (j + rot) % 5: 0 finite, 1 NaN, 2 +Inf, 3 -Inf,
    4 Inf + (-Inf).  Finite neighbours sit between the special ones."""
    a, b = (x.clone() for x in _scaled_inputs(name, n, 2))
    case = (torch.arange(n) + rot) % 5
    a[case == 1] = float("nan")
    a[case == 2] = float("inf")
    b[case == 3] = float("-inf")
    a[case == 4] = float("inf")
    b[case == 4] = float("-inf")
    return a, b, case


@needs_gpu
@pytest.mark.parametrize("rot", [0, 2])
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_fedavg_reduce_non_finite(ext, name, rot):
    """NaN, +-Inf and Inf-Inf in the vector body and (over the two rotations)
    every case in the 3-element tail; finite neighbours keep the bound."""
    n = 5 * VEC[name] + 3
    a, b, case = _nonfinite_inputs(name, n, rot)
    w = [0.3, 0.7]
    out = _reduce(ext, name, [a, b], w)
    _check_weighted_sum(out, [a, b], _w32(w), name)
    o = out.double()
    assert torch.isnan(o[(case == 1) | (case == 4)]).all()
    assert (o[case == 2] == float("inf")).all()
    assert (o[case == 3] == float("-inf")).all()
    assert torch.isfinite(o[case == 0]).all()


@needs_gpu
def test_fedavg_reduce_rejects_bad_arguments(ext):
    def t(n, dt=torch.bfloat16):
        return torch.zeros(n, dtype=dt, device="cuda")

    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_(t(8), [t(8)] * 17, [1.0] * 17)
    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_(t(8), [t(8), t(8, torch.float16)], [0.5, 0.5])
    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_(t(8, torch.int64), [t(8, torch.int64)], [1.0])
    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_(t(8), [t(8), t(9)], [0.5, 0.5])
    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_(t(8), [t(8), t(8)], [0.5])
    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_(t(8), [], [])


@needs_gpu
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("name", ["bf16", "fp16", "fp32"])
def test_fedavg_reduce_misaligned_views(ext, name, off):
    """Contiguous slices at odd element offsets (not 16-byte aligned) for out
    alone, one input alone, and everything: bit-equal to the aligned call and
    nothing outside the view is written."""
    dt = DTYPES[name]
    w = [0.3, 0.7]
    for n in (VEC[name] + 1, 4101):
        a_cpu, b_cpu = _scaled_inputs(name, n, 2)
        a, b = a_cpu.cuda(), b_cpu.cuda()
        ref = torch.empty(n, dtype=dt, device="cuda")
        ext.fedavg_reduce_(ref, [a, b], w)

        def shifted(x):
            buf = torch.zeros(n + 8, dtype=dt, device="cuda")
            buf[off : off + n] = x
            return buf[off : off + n]

        for mis_out, mis_a, mis_b in [(1, 0, 0), (0, 1, 0), (1, 1, 1)]:
            obuf = torch.full((n + 8,), 7.0, dtype=dt, device="cuda")
            o = off if mis_out else 0
            out = obuf[o : o + n]
            ins = [shifted(a) if mis_a else a, shifted(b) if mis_b else b]
            if mis_out:
                assert out.data_ptr() % 16 != 0
            ext.fedavg_reduce_(out, ins, w)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out), _bits(ref)), (n, mis_out, mis_a, mis_b)
            assert (obuf[:o] == 7.0).all() and (obuf[o + n :] == 7.0).all()


# ------------------------------------------------------------ MFMA reduce
# The MFMA unit sums its 32 products inside one instruction rather than as k
# IEEE fp32 additions, so this kernel alone could justify a wider accumulation
# term (up to 2^-18 * S would still separate truncation, ~2^-8 relative, and a
# second bf16 rounding, ~2^-9).  It is not needed: None keeps the same derived
# (k+1) * 2^-23 * S as the VALU kernel, and the test prints the margin.
MFMA_FACTOR = None


@needs_gpu
@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 16])
def test_fedavg_reduce_mfma_half_ulp(ext, k):
    """Weights are rounded to bf16 by the kernel, so the reference uses the
    rounded weights.  n = 262,144 + 17 is a second sweep of 16,384 waves x 16
    plus a partial tile; k = 8, 9 straddle the 8-wide lane groups."""
    worst = 0.0
    for n in (1, 15, 16, 17, 262_144 + 17):
        ins = _scaled_inputs("bf16", n, k)
        w = [(i + 1) / (k * (k + 1) / 2) for i in range(k)]  # not dyadic
        out = _reduce(ext, "bf16", ins, w, mfma=True)
        worst = max(
            worst,
            _check_weighted_sum(out, ins, _wbf16(w), "bf16", factor=MFMA_FACTOR),
        )
    print(f"\nmfma k={k}: worst error beyond half an ulp = {worst:.3e} * S "
          f"(bound {(k + 1) * 2.0 ** -23:.3e})")


@needs_gpu
def test_fedavg_reduce_mfma_rejects_k17(ext):
    x = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ext.fedavg_reduce_mfma_(x.clone(), [x] * 17, [1.0] * 17)


@needs_gpu
@pytest.mark.parametrize("k", [2, 9])
def test_fedavg_reduce_mfma_non_finite_stays_in_its_element(ext, k):
    n = 262_144 + 17
    ins = [x.clone() for x in _scaled_inputs("bf16", n, k)]
    w = [1.0 / k] * k
    clean = _reduce(ext, "bf16", ins, w, mfma=True)
    pos = [0, 5, 15, 16, 4097, 262_144 + 3, n - 1]  # tiles, second sweep, tail
    vals = [float("nan"), float("inf"), float("-inf")]
    for i, p in enumerate(pos):
        ins[i % k][p] = vals[i % 3]
    ins[0][100] = float("inf")
    ins[1][100] = float("-inf")
    pos.append(100)
    dirty = _reduce(ext, "bf16", ins, w, mfma=True)
    _check_weighted_sum(dirty, ins, _wbf16(w), "bf16", factor=MFMA_FACTOR)
    keep = torch.ones(n, dtype=torch.bool)
    keep[pos] = False
    assert torch.equal(_bits(dirty)[keep], _bits(clean)[keep])
    assert not torch.isfinite(dirty.float()[pos]).any()


# ------------------------------------------------------- combine + hash
COMBINE_SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 8_388_608 + 19]


def _combine(ext, local, peer, wa, wb):
    lo, pe = local.cuda(), peer.cuda()
    out = torch.empty_like(lo)
    hv = ext.fedavg_combine_hash_async(out, lo, pe.view(torch.uint8), wa, wb)
    torch.cuda.synchronize()
    want = hash64_ref(_bf16_bits(peer).tobytes())
    assert (int(hv.item()) & M64) == want, "hash of the peer bytes"
    return out.cpu()


@needs_gpu
@pytest.mark.parametrize("n", COMBINE_SIZES)
def test_combine_hash_exact_for_dyadic_weights(ext, n):
    """2^-6-grid inputs, weights 1/4 and 3/4: exact in fp32, so the output is
    rne_bf16(float64 sum) bit for bit.  The last size is a second slot sweep
    with a partial group of words and a tail."""
    g = torch.Generator().manual_seed(n % 1000 + 1)
    local = (torch.randint(-255, 256, (n,), generator=g).double() / 64).bfloat16()
    peer = (torch.randint(-255, 256, (n,), generator=g).double() / 64).bfloat16()
    if n >= 4:  # the tie constructions: 1 + 2^-8 -> 1 and 1 + 3*2^-8 -> 1 + 2^-6
        local[0], peer[0] = 1.0, 1.0 + 2.0 ** -7
        local[n - 1], peer[n - 1] = 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6
        out = _combine(ext, local, peer, 0.5, 0.5)
        assert out[0].item() == 1.0 and out[n - 1].item() == 1.0 + 2.0 ** -6
    out = _combine(ext, local, peer, 0.25, 0.75)
    ref = 0.25 * _f64(local) + 0.75 * _f64(peer)
    exp = torch.from_numpy(_rne(ref, "bf16")).bfloat16()
    assert torch.equal(_bits(out), _bits(exp))


@needs_gpu
@pytest.mark.parametrize("n", [1, 5, 17, 4101])
def test_combine_hash_half_ulp_for_other_weights(ext, n):
    local, peer = _scaled_inputs("bf16", n, 2)
    out = _combine(ext, local, peer, 0.3, 0.7)
    _check_weighted_sum(out, [local, peer], _w32([0.3, 0.7]), "bf16")


@needs_gpu
@pytest.mark.parametrize("rot", [0, 2])
def test_combine_hash_non_finite(ext, rot):
    """NaN / Inf in local and in peer, in whole words and in the 3-element
    tail handled by lane 0."""
    n = 16 + 3
    a, b, case = _nonfinite_inputs("bf16", n, rot)
    for local, peer in ((a, b), (b, a)):
        out = _combine(ext, local, peer, 0.3, 0.7)
        _check_weighted_sum(out, [local, peer], _w32([0.3, 0.7]), "bf16")


@needs_gpu
def test_combine_hash_rejects_misaligned(ext):
    n = 64
    buf = torch.zeros(n + 8, dtype=torch.bfloat16, device="cuda")
    ok = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    okb = ok.view(torch.uint8)
    mis = buf[1 : 1 + n]
    misb = buf.view(torch.uint8)[2 : 2 + 2 * n]
    with pytest.raises(RuntimeError):
        ext.fedavg_combine_hash_async(mis, ok, okb, 0.5, 0.5)
    with pytest.raises(RuntimeError):
        ext.fedavg_combine_hash_async(ok.clone(), mis, okb, 0.5, 0.5)
    with pytest.raises(RuntimeError):
        ext.fedavg_combine_hash_async(ok.clone(), ok, misb, 0.5, 0.5)
    torch.cuda.synchronize()
    assert (buf == 0).all()


# ------------------------------------------------------------------ hash64
@pytest.fixture(scope="module")
def hash_data():
    """2*W + 13 random bytes, on the device and on the host."""
    g = torch.Generator().manual_seed(64)
    cpu = torch.randint(0, 256, (2 * HASH_W + 13,), dtype=torch.uint8, generator=g)
    return cpu.cuda(), cpu.numpy()


@needs_gpu
@pytest.mark.parametrize(
    "n", [HASH_W - 8, HASH_W, HASH_W + 8, HASH_W + 8 * 14 + 5, 2 * HASH_W + 13]
)
def test_hash64_and_pack_across_the_slot_wrap(ext, hash_data, n):
    """Sizes around one full sweep of the 4*524288 word slots: the second
    sweep (base += slots) against the numpy reference."""
    dev, host = hash_data
    want = hash64_ref(host[:n].tobytes())
    assert (int(ext.hash64_async(dev[:n]).item()) & M64) == want
    dst = torch.full((n + 24,), SENT, dtype=torch.uint8, device="cuda")
    hv = ext.pack_hash64_async(dev[:n], dst)
    torch.cuda.synchronize()
    assert (int(hv.item()) & M64) == want
    assert torch.equal(dst[:n], dev[:n])
    assert (dst[n:] == SENT).all()


@needs_gpu
def test_hash64_rejects_misaligned(ext, hash_data):
    dev, _ = hash_data
    dst = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        ext.hash64_async(dev[1:4097])
    with pytest.raises(RuntimeError):
        ext.pack_hash64_async(dev[1:4097], dst)
    with pytest.raises(RuntimeError):
        ext.pack_hash64_async(dev[:4000], dst[3:4003])


# ------------------------------------------------------------------- CRC32
@needs_gpu
@pytest.mark.parametrize("n", [1, 4095, 4096, 3 * 4096 + 5])
@pytest.mark.parametrize("k", [1, 7, 8, 15])
def test_crc32_unaligned_views(ext, k, n):
    """data[k:] is not 16-byte aligned: every slice takes the byte loop."""
    g = torch.Generator().manual_seed(k * 100003 + n)
    cpu = torch.randint(0, 256, (k + n,), dtype=torch.uint8, generator=g)
    view = cpu.cuda()[k:]
    assert view.data_ptr() % 16 != 0
    want = zlib.crc32(cpu.numpy()[k:].tobytes()) & 0xFFFFFFFF
    assert (ext.crc32(view) & 0xFFFFFFFF) == want


@needs_gpu
def test_crc32_64mib_reaches_high_shift_powers(ext):
    """n = 2^26 + 4097: 16,386 slices, so the per-slice shift uses the
    squared matrices up to M^(2^14)."""
    n = (1 << 26) + 4097
    g = torch.Generator().manual_seed(26)
    cpu = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    want = zlib.crc32(cpu.numpy().tobytes()) & 0xFFFFFFFF
    assert (ext.crc32(cpu.cuda()) & 0xFFFFFFFF) == want


@needs_gpu
@pytest.mark.parametrize("n", [1, 15, 17, 4097])
def test_pack_crc_small_sizes(ext, n):
    g = torch.Generator().manual_seed(n)
    cpu = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    src = cpu.cuda()
    dst = torch.full((n + 40,), SENT, dtype=torch.uint8, device="cuda")
    out = ext.pack_crc_async(src, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst[:n], src)
    assert (dst[n:] == SENT).all()
    want = zlib.crc32(cpu.numpy().tobytes()) & 0xFFFFFFFF
    assert (int(out[2].item()) & 0xFFFFFFFF) == want
    # Misaligned src: byte-by-byte copy, to a misaligned dst as well.
    wide = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    wide[3 : 3 + n] = src
    dst2 = torch.full((n + 40,), SENT, dtype=torch.uint8, device="cuda")
    out2 = ext.pack_crc_async(wide[3 : 3 + n], dst2[5 : 5 + n])
    torch.cuda.synchronize()
    assert torch.equal(dst2[5 : 5 + n], src)
    assert (dst2[:5] == SENT).all() and (dst2[5 + n :] == SENT).all()
    assert (int(out2[2].item()) & 0xFFFFFFFF) == want
    # Aligned src takes 16-byte stores: a misaligned dst is rejected.
    with pytest.raises(RuntimeError):
        ext.pack_crc_async(src, dst2[5 : 5 + n])


# -------------------------------------------------------------- masked_add_
@needs_gpu
@pytest.mark.parametrize("mask_kind", ["zero", "one", "random", "random_bool"])
@pytest.mark.parametrize("n", [1, 255, GRID + 1])
@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_masked_add_bit_exact(ext, name, n, mask_kind):
    """Where the mask is set: rne(float32(dst) + float32(src)) bit for bit
    (the float32 sum is IEEE on the CPU; the bf16 rounding is integer math).
    Elsewhere dst keeps its bits."""
    g = torch.Generator().manual_seed(n + len(mask_kind))
    dst0 = torch.randn(n, generator=g).to(DTYPES[name])
    src = torch.randn(n, generator=g).to(DTYPES[name])
    if mask_kind == "zero":
        mask = torch.zeros(n, dtype=torch.uint8)
    elif mask_kind == "one":
        mask = torch.ones(n, dtype=torch.uint8)
    else:
        mask = (torch.rand(n, generator=g) > 0.5).to(torch.uint8)
    if mask_kind == "random_bool":
        mask = mask.bool()
    dst = dst0.cuda()
    ext.masked_add_(dst, src.cuda(), mask.cuda())
    torch.cuda.synchronize()
    s = dst0.float().numpy() + src.float().numpy()  # float32 add
    if name == "bf16":
        summed = _f32_to_bf16_bits(s)
        before = _bf16_bits(dst0)
        got = _bf16_bits(dst)
    else:
        summed = s.view(np.uint32)
        before = dst0.numpy().view(np.uint32)
        got = dst.cpu().numpy().view(np.uint32)
    m = mask.numpy().astype(bool)
    assert np.array_equal(got, np.where(m, summed, before))


@needs_gpu
def test_masked_add_rejects_bad_arguments(ext):
    def t(n, dt=torch.float32, dev="cuda"):
        return torch.zeros(n, dtype=dt, device=dev)

    m = torch.ones(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):  # src dtype != dst dtype
        ext.masked_add_(t(8), t(8, torch.float16), m)
    with pytest.raises(RuntimeError):
        ext.masked_add_(t(8, torch.bfloat16), t(8), m)
    with pytest.raises(RuntimeError):  # fp16 is not supported
        ext.masked_add_(t(8, torch.float16), t(8, torch.float16), m)
    with pytest.raises(RuntimeError):  # CPU src
        ext.masked_add_(t(8), t(8, dev="cpu"), m)
    with pytest.raises(RuntimeError):  # CPU mask
        ext.masked_add_(t(8), t(8), m.cpu())
    with pytest.raises(RuntimeError):  # length mismatch
        ext.masked_add_(t(8), t(9), m)
    with pytest.raises(RuntimeError):
        ext.masked_add_(t(8), t(8), torch.ones(9, dtype=torch.uint8, device="cuda"))
