"""CPU reference of the fp8 wire format (``wire_dtype='fp8e4m3'``).

OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits.  Exponent field 0
holds the subnormals m * 2^-9; exponent 15 with mantissa 7 (bytes 0x7F and
0xFF) is NaN; there is no infinity, so the largest finite value is
1.75 * 2^8 = 448 (0x7E).

Wire contract, pinned on hardware by tests/test_kernel_edges.py against the
pack_fp8 / unpack_fp8 kernels in csrc/rayfed_hip.hip:

  * encode rounds to nearest, ties to the even mantissa;
  * finite |x| > 448 saturates to 0x7E / 0xFE;
  * +-Inf and NaN become the NaN byte ``sign | 0x7F``;
  * the sign of zero is kept;
  * decode is exact, and a NaN byte decodes to NaN.

numpy only, float64/integer math; shares no code with the kernels or torch.
"""
from __future__ import annotations

import numpy as np

MAX_FINITE = 448.0
NAN_BYTE = 0x7F


def _magnitudes() -> np.ndarray:
    """The 127 non-negative finite values, indexed by their byte 0x00..0x7E."""
    b = np.arange(0x7F)
    e = b >> 3
    m = b & 7
    sub = m * 2.0 ** -9
    nrm = (8 + m) * 2.0 ** (e.astype(np.float64) - 10)  # (1 + m/8) * 2^(e-7)
    return np.where(e == 0, sub, nrm)


_MAG = _magnitudes()


def decode(data) -> np.ndarray:
    """fp8 e4m3fn bytes -> float64 (exact)."""
    b = np.asarray(data, dtype=np.uint8)
    mag_bits = b & 0x7F
    out = _MAG[np.minimum(mag_bits, 0x7E)].copy()
    out[mag_bits == NAN_BYTE] = np.nan
    return np.where((b & 0x80) != 0, -out, out)


def encode(x) -> np.ndarray:
    """float64 -> fp8 e4m3fn bytes (RNE, saturating, non-finite -> NaN byte)."""
    x = np.asarray(x, dtype=np.float64)
    sign = np.where(np.signbit(x), 0x80, 0).astype(np.uint8)
    finite = np.isfinite(x)
    a = np.where(finite, np.abs(x), 0.0)
    a = np.minimum(a, MAX_FINITE)
    # Nearest representable magnitude: lo <= a <= hi are neighbouring bytes.
    hi = np.minimum(np.searchsorted(_MAG, a, side="left"), 0x7E)
    lo = np.maximum(hi - 1, 0)
    d_lo = a - _MAG[lo]
    d_hi = _MAG[hi] - a
    # Consecutive bytes alternate mantissa parity, so on a tie pick the even
    # byte; an exact hit has d_hi == 0 and lands on hi.
    pick_hi = (d_hi < d_lo) | ((d_hi == d_lo) & ((hi & 1) == 0))
    mag = np.where(pick_hi, hi, lo).astype(np.uint8)
    mag = np.where(finite, mag, np.uint8(NAN_BYTE)).astype(np.uint8)
    return sign | mag
