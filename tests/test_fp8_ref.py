"""CPU tests of the fp8 wire reference (rayfed_amd/ops/fp8_ref.py) against
torch's own float8_e4m3fn casts, plus hand-derived pins where the wire
contract (saturate, non-finite -> NaN byte) differs from torch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from rayfed_amd.ops import fp8_ref  # noqa: E402


def _all_bf16():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16)


def test_encode_matches_torch_on_every_in_range_bf16():
    x = _all_bf16()
    xf = x.double().numpy()
    got = fp8_ref.encode(xf)
    want = x.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    in_range = np.isfinite(xf) & (np.abs(xf) <= 448.0)
    assert in_range.sum() == 34754
    bad = np.flatnonzero(in_range & (got != want))
    assert bad.size == 0, [(hex(i), hex(got[i]), hex(want[i])) for i in bad[:8]]


def test_encode_out_of_range_and_non_finite():
    x = _all_bf16().double().numpy()
    got = fp8_ref.encode(x)
    sign = np.where(np.signbit(x), 0x80, 0)
    big = np.isfinite(x) & (np.abs(x) > 448.0)
    assert np.array_equal(got[big], (sign[big] | 0x7E).astype(np.uint8))
    nonfin = ~np.isfinite(x)
    assert np.array_equal(got[nonfin], (sign[nonfin] | 0x7F).astype(np.uint8))


def test_decode_matches_torch_on_every_byte():
    b = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = b.view(torch.float8_e4m3fn).to(torch.bfloat16)
    got = fp8_ref.decode(b.numpy())
    want_f = want.double().numpy()
    nan = np.isnan(got)
    assert np.array_equal(nan, np.isnan(want_f))
    assert sorted(np.flatnonzero(nan).tolist()) == [0x7F, 0xFF]
    assert np.array_equal(got[~nan], want_f[~nan])
    # Sign bits (incl. -0.0 at 0x80); a NaN's sign carries no meaning and
    # torch's expansion of 0xFF drops it.
    assert np.array_equal(np.signbit(got[~nan]), np.signbit(want_f[~nan]))
    assert np.signbit(got[0x80]) and got[0x80] == 0.0
    # Every decode is exactly representable in bf16 (the kernels' output type).
    back = torch.from_numpy(got[~nan]).to(torch.bfloat16).double().numpy()
    assert np.array_equal(back, got[~nan])


def test_roundtrip_is_identity_on_bytes():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(fp8_ref.encode(fp8_ref.decode(b)), b)


@pytest.mark.parametrize(
    "x, byte",
    [
        (2.0 ** -10, 0x00),  # tie between 0 and the smallest subnormal -> even
        (3 * 2.0 ** -10, 0x02),  # tie between 0x01 and 0x02 -> even
        (5 * 2.0 ** -10, 0x02),  # tie between 0x02 and 0x03 -> even
        (2.0 ** -9, 0x01),
        (7 * 2.0 ** -9, 0x07),  # largest subnormal
        (2.0 ** -6, 0x08),  # smallest normal
        (15 * 2.0 ** -10, 0x08),  # tie between 0x07 and 0x08 -> even
        (1.0, 0x38),
        (1.0625, 0x38),  # tie 1 / 1.125 -> even mantissa 0
        (1.1875, 0x3A),  # tie 1.125 / 1.25 -> even mantissa 2
        (448.0, 0x7E),
        (464.0, 0x7E),
        (1e30, 0x7E),
        (-1e30, 0xFE),
        (0.0, 0x00),
        (-0.0, 0x80),
        (-(2.0 ** -10), 0x80),
        (float("inf"), 0x7F),
        (float("-inf"), 0xFF),
    ],
)
def test_encode_pins(x, byte):
    assert int(fp8_ref.encode(np.array([x]))[0]) == byte


def test_encode_nan_keeps_sign():
    pos = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)
    neg = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)
    assert int(fp8_ref.encode(pos.astype(np.float64))[0]) == 0x7F
    assert int(fp8_ref.encode(neg.astype(np.float64))[0]) == 0xFF


def test_decode_pins():
    d = fp8_ref.decode(np.array([0x00, 0x80, 0x01, 0x07, 0x08, 0x38, 0x7E, 0xFE],
                                dtype=np.uint8))
    assert d.tolist() == [0.0, -0.0, 2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -6, 1.0,
                          448.0, -448.0]
    assert np.signbit(d[1]) and not np.signbit(d[0])
