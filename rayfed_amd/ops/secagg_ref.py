"""CPU reference of pairwise-mask secure aggregation in the ring Z/2^32.

This module is the specification, the CPU path of
:mod:`rayfed_amd.parallel.secagg`, and the oracle the HIP kernels
(csrc/secagg_kernels.h) are pinned against bit-for-bit on hardware
(tests/test_secagg_gpu.py).  Every step below is exact; nothing is
"close enough".

Parties are ordered by sorted name; ``idx(p)`` is a party's position in
that order.  At most 16 parties.

Quantise
    ``q(x) = sat_i32(rint(fl32(fl32(x) * fl32(weight)) * 2^frac_bits))``.
    ``rint`` is round-half-to-even.  ``sat_i32`` clamps to
    [-2^31, 2^31-1] (so +inf -> 2^31-1, -inf -> -2^31); NaN -> 0.
    ``frac_bits`` in [0, 30].  Inputs (fp32/bf16/fp16) are widened exactly
    to fp32 first; both products are plain fp32 multiplies (no FMA) and the
    second, by a power of two, is exact.  The caller must keep
    ``|sum_i w_i x_i| < 2^(31 - frac_bits)`` or the ring sum wraps.

Keystream
    ``KS(key, round, e)`` is word ``e mod 16`` of the ChaCha20 block
    (20 rounds, IETF layout of RFC 8439 section 2.3): the four constants,
    the 32-byte key as 8 little-endian words, 32-bit block counter
    ``e div 16`` (starting at 0), nonce words
    ``(round & 0xffffffff, round >> 32, 0)``.  The counter never wraps:
    ``offset + n <= 2^36`` is validated.

Mask
    ``y_i[e] = q_i[e] + sum_{j != i} s(i,j) * KS(key_ij, round, offset+e)``
    mod 2^32, stored as int32.  ``s(i,j) = +1`` if ``idx(i) < idx(j)`` else
    -1.  ``offset`` is the element index of ``x[0]`` in the logical flat
    vector, a multiple of 16.

Aggregate
    ``S[e] = sum_{i in survivors} y_i[e]
             - sum_{i in survivors, d in dropped} s(i,d) * KS(key_id, ...)``
    mod 2^32; ``out[e] = cast(fl32(int32(S[e])) * 2^-frac_bits)``.  The
    int->fp32 conversion and the cast to fp32/bf16/fp16 are
    round-to-nearest-even.

Differential privacy (optional; clip, then binomial noise before masking)

Noise stream
    ``NS(key, round, w)`` is word ``w mod 16`` of the ChaCha20 block with
    the party's private 32-byte *noise key*, block counter ``w div 16`` and
    nonce words ``(round & 0xffffffff, round >> 32, 1)``.  The third nonce
    word separates it from every pair-mask keystream (which uses 0) even
    if a key were reused.

Binomial noise
    Parameters ``words`` (W) in {1, 2, 4, 8, 16} - an element's words never
    straddle a block - and ``step``, an int in [1, 2^20].  For element ``e``
    of the logical flat vector
    ``noise[e] = step * (sum_{t<W} popcount(NS(key, round, W*e + t)) - 16*W)``
    mod 2^32: ``step * (Bin(32W, 1/2) - 16W)``, variance ``8*W*step^2`` in
    fixed-point units, ``|noise[e]| <= 16*W*step``.  The counter never
    wraps: ``offset % 16 == 0`` and ``(offset + n) * W <= 2^36`` are
    validated.

Mask with noise
    ``y_i[e] = q_i[e] + noise_i[offset+e] + sum_{j != i} s(i,j) * KS(...)``
    mod 2^32.  The noise rides in the ring sum: the aggregate is the
    quantised sum plus the survivors' noises, exactly.  The caller must keep
    ``|sum_i w_i x_i| + 16*W*step*contributors/2^frac_bits
    < 2^(31 - frac_bits)``.

Sum of squares (for L2 clipping)
    ``sum_e float64(x[e])^2`` accumulated in float64.  Every square of an
    fp32/bf16/fp16 value is exact in float64; only the order of the
    additions is unspecified, so two conforming results differ by at most
    ``n * 2^-52`` relative.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

MAX_PARTIES = 16
MAX_FRAC_BITS = 30
MAX_ELEMENTS = 1 << 36  # 2^32 blocks of 16 words: the counter never wraps
NOISE_WORDS = (1, 2, 4, 8, 16)  # keystream words per element
MAX_NOISE_STEP = 1 << 20
NOISE_NONCE_WORD = 1  # third nonce word of the noise stream (masks use 0)
_CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def _key_words(key: bytes) -> np.ndarray:
    if not isinstance(key, (bytes, bytearray)) or len(key) != 32:
        raise ValueError("a secagg pair key must be exactly 32 bytes")
    return np.frombuffer(bytes(key), dtype="<u4")


def _rotl(x: np.ndarray, n: int, tmp: np.ndarray) -> None:
    np.right_shift(x, np.uint32(32 - n), out=tmp)
    np.left_shift(x, np.uint32(n), out=x)
    np.bitwise_or(x, tmp, out=x)


def _quarter(s, a, b, c, d, tmp) -> None:
    s[a] += s[b]; s[d] ^= s[a]; _rotl(s[d], 16, tmp)
    s[c] += s[d]; s[b] ^= s[c]; _rotl(s[b], 12, tmp)
    s[a] += s[b]; s[d] ^= s[a]; _rotl(s[d], 8, tmp)
    s[c] += s[d]; s[b] ^= s[c]; _rotl(s[b], 7, tmp)


def chacha20_blocks(key: bytes, counter0: int, nonce_words: Sequence[int],
                    nblocks: int) -> np.ndarray:
    """``nblocks`` consecutive ChaCha20 blocks as ``uint32[nblocks, 16]``,
    block counters ``counter0 .. counter0+nblocks-1`` (vectorised over
    blocks)."""
    kw = _key_words(key)
    if len(nonce_words) != 3:
        raise ValueError("nonce_words must be three 32-bit words")
    if counter0 < 0 or nblocks < 0 or counter0 + nblocks > (1 << 32):
        raise ValueError("ChaCha20 block counter would wrap")
    init = np.empty((16, nblocks), dtype=np.uint32)
    for i, c in enumerate(_CONSTANTS):
        init[i] = c
    for i in range(8):
        init[4 + i] = kw[i]
    init[12] = (np.arange(nblocks, dtype=np.uint64)
                + np.uint64(counter0)).astype(np.uint32)
    for i in range(3):
        init[13 + i] = int(nonce_words[i]) & 0xFFFFFFFF
    s = init.copy()
    tmp = np.empty(nblocks, dtype=np.uint32)
    rows = list(s)  # row views, updated in place
    for _ in range(10):
        _quarter(rows, 0, 4, 8, 12, tmp)
        _quarter(rows, 1, 5, 9, 13, tmp)
        _quarter(rows, 2, 6, 10, 14, tmp)
        _quarter(rows, 3, 7, 11, 15, tmp)
        _quarter(rows, 0, 5, 10, 15, tmp)
        _quarter(rows, 1, 6, 11, 12, tmp)
        _quarter(rows, 2, 7, 8, 13, tmp)
        _quarter(rows, 3, 4, 9, 14, tmp)
    s += init
    return np.ascontiguousarray(s.T)


def check_range(offset: int, n: int) -> None:
    if offset < 0 or n < 0:
        raise ValueError("offset and length must be non-negative")
    if offset % 16 != 0:
        raise ValueError("secagg offset must be a multiple of 16")
    if offset + n > MAX_ELEMENTS:
        raise ValueError(
            "offset + n exceeds 2^36: the ChaCha20 block counter would wrap")


def check_frac_bits(frac_bits: int) -> None:
    if not isinstance(frac_bits, int) or not 0 <= frac_bits <= MAX_FRAC_BITS:
        raise ValueError(f"frac_bits must be an int in [0, {MAX_FRAC_BITS}]")


def check_round(round: int) -> None:
    if not isinstance(round, int) or not 0 <= round < (1 << 64):
        raise ValueError("round must be an int in [0, 2^64)")


def keystream(key: bytes, round: int, offset: int, n: int) -> np.ndarray:
    """``KS(key, round, offset+e)`` for ``e in [0, n)`` as ``uint32[n]``."""
    check_round(round)
    check_range(offset, n)
    nblocks = (n + 15) // 16
    nonce = (round & 0xFFFFFFFF, round >> 32, 0)
    return chacha20_blocks(key, offset // 16, nonce, nblocks).reshape(-1)[:n]


def quantize(x, weight: float = 1.0, frac_bits: int = 16) -> np.ndarray:
    """Fixed-point quantisation of an fp32 array -> ``int32``."""
    check_frac_bits(frac_bits)
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = x * np.float32(weight)                 # fp32 product
        t = t * np.float32(2.0 ** frac_bits)       # exact (power of two)
        r = np.rint(t).astype(np.float64)          # half-to-even
    r = np.where(np.isnan(r), 0.0, r)
    r = np.clip(r, -2147483648.0, 2147483647.0)
    return r.astype(np.int64).astype(np.int32)


def _signed_keystreams(acc: np.ndarray, keys, signs, round, offset,
                       negate: bool) -> None:
    if len(keys) != len(signs):
        raise ValueError("keys/signs length mismatch")
    for key, sign in zip(keys, signs):
        if sign not in (1, -1):
            raise ValueError("signs must be +1 or -1")
        ks = keystream(key, round, offset, acc.size)
        if (sign > 0) != negate:
            acc += ks
        else:
            acc -= ks


def mask_ref(x, weight: float, frac_bits: int, keys: Sequence[bytes],
             signs: Sequence[int], round: int, offset: int = 0) -> np.ndarray:
    """``y = q(x) + sum_k signs[k] * KS(keys[k], round, offset+e)`` mod 2^32
    as ``int32``."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    check_round(round)
    check_range(offset, x.size)
    acc = quantize(x, weight, frac_bits).view(np.uint32).copy()
    _signed_keystreams(acc, keys, signs, round, offset, negate=False)
    return acc.view(np.int32)


def cast_ref(f: np.ndarray, out_dtype: str) -> np.ndarray:
    """RNE cast of finite fp32 values.  ``bfloat16`` is returned as its
    ``uint16`` bit pattern (numpy has no bf16)."""
    f = np.asarray(f, dtype=np.float32)
    if out_dtype == "float32":
        return f
    if out_dtype == "float16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16)
    if out_dtype == "bfloat16":
        u = f.view(np.uint32)
        r = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
        return (r >> np.uint32(16)).astype(np.uint16)
    raise ValueError(f"unsupported out_dtype {out_dtype!r}")


def ring_sum_ref(masked: Sequence[np.ndarray], corr_keys: Sequence[bytes],
                 corr_signs: Sequence[int], round: int,
                 offset: int = 0) -> np.ndarray:
    """``S = sum_i masked[i] - sum_c corr_signs[c] * KS(corr_keys[c], ...)``
    mod 2^32 as ``int32``."""
    if not masked:
        raise ValueError("aggregate needs at least one masked vector")
    n = np.asarray(masked[0]).size
    check_round(round)
    check_range(offset, n)
    acc = np.zeros(n, dtype=np.uint32)
    for y in masked:
        y = np.asarray(y)
        if y.dtype != np.int32 or y.size != n:
            raise ValueError("masked vectors must be int32 of equal length")
        acc += y.reshape(-1).view(np.uint32)
    _signed_keystreams(acc, corr_keys, corr_signs, round, offset, negate=True)
    return acc.view(np.int32)


def aggregate_ref(masked: Sequence[np.ndarray], corr_keys: Sequence[bytes],
                  corr_signs: Sequence[int], round: int, offset: int = 0,
                  frac_bits: int = 16,
                  out_dtype: str = "float32") -> np.ndarray:
    """Ring sum, residual-mask removal and dequantise (see module doc)."""
    check_frac_bits(frac_bits)
    s = ring_sum_ref(masked, corr_keys, corr_signs, round, offset)
    f = s.astype(np.float32) * np.float32(2.0 ** -frac_bits)
    return cast_ref(f, out_dtype)


# ------------------------------------------------- binomial noise (DP)
def check_noise(words: int, step: int) -> None:
    if isinstance(words, bool) or not isinstance(words, int) \
            or words not in NOISE_WORDS:
        raise ValueError(f"noise words must be one of {NOISE_WORDS}")
    if isinstance(step, bool) or not isinstance(step, int) \
            or not 1 <= step <= MAX_NOISE_STEP:
        raise ValueError("noise step must be an int in [1, 2^20]")


def check_noise_range(offset: int, n: int, words: int) -> None:
    """The noise rule: ``words`` keystream words per element."""
    if offset < 0 or n < 0:
        raise ValueError("offset and length must be non-negative")
    if offset % 16 != 0:
        raise ValueError("secagg offset must be a multiple of 16")
    if (offset + n) * words > MAX_ELEMENTS:
        raise ValueError(
            "(offset + n) * words exceeds 2^36: the ChaCha20 block counter "
            "of the noise stream would wrap")


def _popcount32(v: np.ndarray) -> np.ndarray:
    """Bit count of every uint32 (SWAR; no numpy-version dependence)."""
    v = v - ((v >> np.uint32(1)) & np.uint32(0x55555555))
    v = (v & np.uint32(0x33333333)) + ((v >> np.uint32(2))
                                       & np.uint32(0x33333333))
    v = (v + (v >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return (v * np.uint32(0x01010101)) >> np.uint32(24)


def binomial_noise(key: bytes, round: int, offset: int, n: int, words: int,
                   step: int) -> np.ndarray:
    """``noise[offset+e]`` for ``e in [0, n)`` as ``uint32[n]`` (mod 2^32)."""
    if not isinstance(key, (bytes, bytearray)) or len(key) != 32:
        raise ValueError("a noise key must be exactly 32 bytes")
    check_round(round)
    check_noise(words, step)
    check_noise_range(offset, n, words)
    nblocks = (n * words + 15) // 16
    nonce = (round & 0xFFFFFFFF, round >> 32, NOISE_NONCE_WORD)
    ns = chacha20_blocks(key, offset // 16 * words, nonce, nblocks)
    bits = _popcount32(ns.reshape(-1)[:n * words]).reshape(n, words)
    centred = bits.sum(axis=1, dtype=np.int64) - 16 * words
    return (centred * step).astype(np.uint32)  # two's complement wrap


def mask_noise_ref(x, weight: float, frac_bits: int, keys: Sequence[bytes],
                   signs: Sequence[int], round: int, offset: int,
                   noise_key: bytes, words: int, step: int) -> np.ndarray:
    """``mask_ref(...) + binomial_noise(noise_key, ...)`` mod 2^32 as
    ``int32``."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    noise = binomial_noise(noise_key, round, offset, x.size, words, step)
    y = mask_ref(x, weight, frac_bits, keys, signs, round, offset)
    return (y.view(np.uint32) + noise).view(np.int32)


def sum_squares_ref(x) -> float:
    """Float64 sum of the squares of ``x``'s values widened exactly to
    float64 (NaN / Inf propagate; 0.0 for an empty array)."""
    v = np.asarray(x).astype(np.float64).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(v * v))
