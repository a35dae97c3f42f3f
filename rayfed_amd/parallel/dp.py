"""Differential privacy for secure aggregation: L2 clipping and binomial
noise.

A party clips its update to an L2 bound and adds calibrated noise *before*
masking, so the unmasked aggregate itself is differentially private:

    noise = BinomialNoise.fresh(words=4, step=s)        # private, per party
    w = weight * clip_factor(update_tensors, clip_norm)  # norm of the WHOLE
    y = session.mask(bucket, round=r, weight=w,          # update, then mask
                     offset=off, noise=noise)            # per bucket

The noise is the binomial mechanism: ``step * (popcount of 32*words
keystream bits - 16*words)`` per element, an exact integer in Z/2^32 defined
bit for bit in ``rayfed_amd.ops.secagg_ref`` (the normative spec).  On CUDA
tensors it is generated inside the quantise-and-mask kernel, and the norm is
one read-only pass (``sumsq_kernel``); on CPU tensors both are the numpy
reference.  Sums of binomials are binomial, so ``contributors`` surviving
parties with equal parameters add up to ``step * (Bin(32*words*contributors,
1/2) - 16*words*contributors)``.

There is deliberately no (epsilon, delta) accountant here: the parameters the
binomial-mechanism analysis needs (``std``, ``max_abs``, total bits
``32*words*contributors``, the L2 sensitivity) are exposed; see
docs/secagg.md.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Sequence, Union

import torch

from rayfed_amd.ops import secagg_ref

__all__ = ["BinomialNoise", "sum_squares", "clip_factor"]

_IN_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _check_contributors(contributors: int) -> None:
    if (isinstance(contributors, bool) or not isinstance(contributors, int)
            or contributors < 1):
        raise ValueError("contributors must be a positive int")


@dataclass(frozen=True)
class BinomialNoise:
    """One party's binomial-noise parameters and its private 32-byte key.

    ``words`` (1, 2, 4, 8 or 16) is the number of 32-bit keystream words
    whose bits are counted per element; ``step`` (1 .. 2^20) scales the
    centred count, in fixed-point units of ``2^-frac_bits``.  The key never
    leaves the party; a fresh one per session (``fresh``) is the normal use.
    Never reuse a ``(key, round)`` pair for two different vectors at
    overlapping offsets.
    """

    key: bytes = field(repr=False)
    words: int = 4
    step: int = 1

    def __post_init__(self):
        if not isinstance(self.key, (bytes, bytearray)) or len(self.key) != 32:
            raise ValueError("a noise key must be exactly 32 bytes")
        object.__setattr__(self, "key", bytes(self.key))
        secagg_ref.check_noise(self.words, self.step)

    @classmethod
    def fresh(cls, words: int = 4, step: int = 1) -> "BinomialNoise":
        """Parameters with a key drawn from ``os.urandom``."""
        return cls(os.urandom(32), words, step)

    def std(self, frac_bits: int, contributors: int = 1) -> float:
        """Standard deviation, in the update's units, of the summed noise of
        ``contributors`` parties: ``step*sqrt(8*words*contributors) /
        2^frac_bits``."""
        secagg_ref.check_frac_bits(frac_bits)
        _check_contributors(contributors)
        return (self.step * math.sqrt(8 * self.words * contributors)
                / 2.0 ** frac_bits)

    def max_abs(self, frac_bits: int, contributors: int = 1) -> float:
        """Largest magnitude of that sum: ``16*words*step*contributors /
        2^frac_bits`` — the headroom the overflow rule must leave."""
        secagg_ref.check_frac_bits(frac_bits)
        _check_contributors(contributors)
        return 16 * self.words * self.step * contributors / 2.0 ** frac_bits


def _as_list(tensors) -> Sequence[torch.Tensor]:
    if isinstance(tensors, torch.Tensor):
        return [tensors]
    ts = list(tensors)
    for t in ts:
        if not isinstance(t, torch.Tensor):
            raise ValueError("sum_squares takes a tensor or a sequence of "
                             "tensors")
    return ts


def sum_squares(tensors: Union[torch.Tensor, Sequence[torch.Tensor]]
                ) -> float:
    """Float64 sum of the squares of every element of one tensor or a
    sequence of tensors (fp32 / bf16 / fp16).  CUDA tensors are summed by
    the HIP kernel with a single host read-back for the whole sequence; CPU
    tensors by the numpy reference.  NaN and Inf propagate."""
    total = 0.0
    parts = []
    for t in _as_list(tensors):
        if t.dtype not in _IN_DTYPES:
            raise ValueError(f"unsupported dtype {t.dtype}")
        if t.is_cuda:
            if not t.is_contiguous():
                raise ValueError("CUDA tensors must be contiguous")
            from rayfed_amd.ops import _hip_loader

            with torch.cuda.device(t.device):
                parts.append(_hip_loader.load().sumsq_async(
                    t.detach().view(-1)))
        else:
            total += secagg_ref.sum_squares_ref(
                t.detach().to(torch.float64).numpy())
    if parts:
        first = parts[0].device
        host = torch.cat([p.to(first) for p in parts]).cpu()
        for v in host.tolist():
            total += v
    return total


def clip_factor(tensors: Union[torch.Tensor, Sequence[torch.Tensor]],
                clip_norm: float) -> float:
    """``min(1.0, clip_norm / ||update||_2)`` over all of ``tensors`` — the
    factor a party multiplies its ``weight`` by so that the weighted update
    has L2 norm at most ``weight * clip_norm``.  Because the norm is over
    the whole update, clipping stays correct when ``mask`` is then called
    per bucket with an ``offset``.  1.0 for a zero update; ``ValueError`` if
    the norm is not finite or ``clip_norm <= 0``."""
    clip_norm = float(clip_norm)
    if not clip_norm > 0.0 or math.isinf(clip_norm):
        raise ValueError("clip_norm must be a positive finite number")
    ss = sum_squares(tensors)
    if not math.isfinite(ss):
        raise ValueError("the update's sum of squares is not finite "
                         "(NaN or Inf element)")
    if ss == 0.0:
        return 1.0
    return min(1.0, clip_norm / math.sqrt(ss))
