"""Secure aggregation: pairwise ChaCha20 masks in the ring Z/2^32.

Each party quantises its (weighted) update to fixed point and adds, for
every peer, a keystream expanded from the pair's 32-byte key — with
opposite signs at the two ends of a pair.  The masks cancel **bit-exactly**
in the ring sum, so the aggregating party learns only the aggregate
(honest-but-curious aggregator; Bonawitz et al. style, without the
self-mask / secret-sharing layers).  If a party drops out, every survivor
reveals the key it shared with the dropped party and the aggregator removes
the residual masks.

On CUDA tensors masking and aggregation are the HIP kernels in
``csrc/secagg_kernels.h``; on CPU tensors they are the numpy reference
``rayfed_amd.ops.secagg_ref``, whose module docstring is the normative
specification.  Both produce identical bits.

The caller must keep ``|sum_i w_i x_i| < 2^(31 - frac_bits)`` for every
element, or the ring sum wraps.  With differential-privacy noise
(``mask(..., noise=BinomialNoise(...))``, see :mod:`rayfed_amd.parallel.dp`)
the rule is ``|sum_i w_i x_i| + noise.max_abs(frac_bits, contributors)
< 2^(31 - frac_bits)``.  The noise rides in the ring sum, so ``aggregate``
is unchanged; a dropped party's noise is absent from the sum, so each party
should size its share for the smallest number of survivors it is willing to
accept.  Key agreement is out of scope: a session
takes a ``{peer: key}`` mapping.  :func:`derive_pair_key` /
:meth:`SecAggSession.from_shared_secret` derive pair keys from one secret
known to all parties — a convenience for tests and demos, NOT a key
exchange (anyone holding the secret can unmask every update).
"""
from __future__ import annotations

import hashlib
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from rayfed_amd.ops import secagg_ref
from rayfed_amd.parallel.dp import BinomialNoise

__all__ = ["SecAggSession", "aggregate", "derive_pair_key"]

_IN_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_DTYPE_NAMES = {
    torch.float32: "float32",
    torch.bfloat16: "bfloat16",
    torch.float16: "float16",
}
_KEY_DOMAIN = b"rayfed-secagg-v1\0"


def derive_pair_key(secret: bytes, a: str, b: str) -> bytes:
    """``SHA-256(b"rayfed-secagg-v1\\0" + secret + b"\\0" + min(a,b) +
    b"\\0" + max(a,b))`` — shared-secret provisioning, not a key exchange."""
    if isinstance(secret, str):
        secret = secret.encode()
    lo, hi = sorted((a, b))
    return hashlib.sha256(
        _KEY_DOMAIN + bytes(secret) + b"\0" + lo.encode() + b"\0" + hi.encode()
    ).digest()


def _ordered(parties: Iterable[str]) -> List[str]:
    order = sorted(parties)
    if len(set(order)) != len(order):
        raise ValueError("duplicate party names")
    if not order:
        raise ValueError("secagg needs at least one party")
    if len(order) > secagg_ref.MAX_PARTIES:
        raise ValueError(
            f"secagg supports at most {secagg_ref.MAX_PARTIES} parties")
    return order


def _check_key(key, who: str) -> bytes:
    if not isinstance(key, (bytes, bytearray)) or len(key) != 32:
        raise ValueError(f"pair key for {who} must be exactly 32 bytes")
    return bytes(key)


def _sign(order: Sequence[str], i: str, j: str) -> int:
    """s(i,j) = +1 if idx(i) < idx(j) else -1."""
    return 1 if order.index(i) < order.index(j) else -1


def _key_tensors(keys: Sequence[bytes],
                 signs: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    kt = torch.from_numpy(
        np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
    ).reshape(len(keys), 32)
    return kt, torch.tensor(list(signs), dtype=torch.int32)


def _flat(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch.Tensor")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t.view(-1)


class SecAggSession:
    """One party's view of a secure-aggregation group.

    ``pair_keys`` maps every other party to the 32-byte key shared with it.
    """

    def __init__(self, parties: Iterable[str], me: str,
                 pair_keys: Mapping[str, bytes], frac_bits: int = 16):
        self._order = _ordered(parties)
        if me not in self._order:
            raise ValueError(f"party {me!r} is not in {self._order}")
        secagg_ref.check_frac_bits(frac_bits)
        self._me = me
        self._frac_bits = frac_bits
        self._peers = [p for p in self._order if p != me]
        self._keys: Dict[str, bytes] = {}
        for p in self._peers:
            if p not in pair_keys:
                raise ValueError(f"no pair key for peer {p!r}")
            self._keys[p] = _check_key(pair_keys[p], repr(p))
        for p in pair_keys:
            if p not in self._keys:
                raise ValueError(f"pair key given for unknown peer {p!r}")
        self._signs = [_sign(self._order, me, p) for p in self._peers]
        self._key_t, self._sign_t = _key_tensors(
            [self._keys[p] for p in self._peers], self._signs)

    @classmethod
    def from_shared_secret(cls, parties: Iterable[str], me: str, secret: bytes,
                           frac_bits: int = 16) -> "SecAggSession":
        """Derive every pair key from one shared secret (tests and demos;
        not a key exchange)."""
        order = _ordered(parties)
        keys = {p: derive_pair_key(secret, me, p) for p in order if p != me}
        return cls(order, me, keys, frac_bits)

    @property
    def parties(self) -> List[str]:
        return list(self._order)

    @property
    def frac_bits(self) -> int:
        return self._frac_bits

    def mask(self, x: torch.Tensor, round: int, weight: float = 1.0,
             offset: int = 0, out: Optional[torch.Tensor] = None,
             noise: Optional[BinomialNoise] = None) -> torch.Tensor:
        """Quantise ``weight * x`` and add this party's pairwise masks for
        ``round``; returns an int32 tensor of ``x``'s shape.  ``offset`` is
        the element index of ``x[0]`` in the logical flat vector (multiple
        of 16), so bucket or chunk views can be masked independently.

        ``noise`` adds this party's binomial noise (differential privacy,
        see :mod:`rayfed_amd.parallel.dp`) to the quantised update before
        the masks, in the same pass; ``(offset + n) * noise.words <= 2^36``
        must then hold.  ``None`` is the plain path, bit for bit."""
        xf = _flat(x, "x")
        if xf.dtype not in _IN_DTYPES:
            raise ValueError(f"unsupported dtype {x.dtype}")
        secagg_ref.check_round(round)
        if noise is None:
            secagg_ref.check_range(offset, xf.numel())
        elif not isinstance(noise, BinomialNoise):
            raise ValueError("noise must be a BinomialNoise or None")
        else:
            secagg_ref.check_noise_range(offset, xf.numel(), noise.words)
        if out is None:
            out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
        of = _flat(out, "out")
        if (of.dtype != torch.int32 or of.device != xf.device
                or of.numel() != xf.numel()):
            raise ValueError(
                "out must be an int32 tensor of x's length on x's device")
        if xf.is_cuda:
            from rayfed_amd.ops import _hip_loader

            with torch.cuda.device(xf.device):
                if noise is None:
                    _hip_loader.load().secagg_mask_async(
                        xf, of, self._key_t, self._sign_t, round, offset,
                        float(weight), self._frac_bits)
                else:
                    nk = torch.frombuffer(bytearray(noise.key),
                                          dtype=torch.uint8)
                    _hip_loader.load().secagg_mask_noise_async(
                        xf, of, self._key_t, self._sign_t, nk, noise.words,
                        noise.step, round, offset, float(weight),
                        self._frac_bits)
            return out
        keys = [self._keys[p] for p in self._peers]
        if noise is None:
            y = secagg_ref.mask_ref(
                xf.float().numpy(), float(weight), self._frac_bits, keys,
                self._signs, round, offset)
        else:
            y = secagg_ref.mask_noise_ref(
                xf.float().numpy(), float(weight), self._frac_bits, keys,
                self._signs, round, offset, noise.key, noise.words,
                noise.step)
        of.copy_(torch.from_numpy(y))
        return out

    def reveal(self, dropped: Iterable[str]) -> Dict[str, bytes]:
        """The pair keys this (surviving) party shared with each dropped
        party — what it sends the aggregator so the residual masks can be
        removed."""
        res = {}
        for d in dropped:
            if d == self._me or d not in self._keys:
                raise ValueError(f"{d!r} is not a peer of {self._me!r}")
            res[d] = self._keys[d]
        return res


def aggregate(masked: Mapping[str, torch.Tensor], parties: Iterable[str],
              round: int, frac_bits: int = 16,
              out_dtype: torch.dtype = torch.float32,
              revealed: Optional[Mapping[str, Mapping[str, bytes]]] = None,
              offset: int = 0, out: Optional[torch.Tensor] = None
              ) -> torch.Tensor:
    """Unmask the sum of the survivors' masked vectors and dequantise.

    Parties of ``parties`` absent from ``masked`` are the dropped set;
    ``revealed`` is ``{survivor: {dropped: key}}`` and must hold exactly one
    key per (survivor, dropped) pair.
    """
    order = _ordered(parties)
    secagg_ref.check_frac_bits(frac_bits)
    secagg_ref.check_round(round)
    if out_dtype not in _DTYPE_NAMES:
        raise ValueError(f"unsupported out_dtype {out_dtype}")
    for p in masked:
        if p not in order:
            raise ValueError(f"masked vector from unknown party {p!r}")
    survivors = [p for p in order if p in masked]
    dropped = [p for p in order if p not in masked]
    if not survivors:
        raise ValueError("aggregate needs at least one masked vector")

    revealed = revealed or {}
    for s in revealed:
        if s not in survivors:
            raise ValueError(f"revealed keys from non-survivor {s!r}")
    corr_keys: List[bytes] = []
    corr_signs: List[int] = []
    for s in survivors:
        got = dict(revealed.get(s, {}))
        for d in dropped:
            if d not in got:
                raise ValueError(
                    f"missing revealed key of survivor {s!r} for dropped "
                    f"party {d!r}")
            corr_keys.append(_check_key(got.pop(d), f"({s!r}, {d!r})"))
            corr_signs.append(_sign(order, s, d))
        if got:
            raise ValueError(
                f"survivor {s!r} revealed keys for parties that did not "
                f"drop: {sorted(got)}")

    flats = [_flat(masked[p], f"masked[{p!r}]") for p in survivors]
    first = flats[0]
    for t in flats:
        if t.dtype != torch.int32:
            raise ValueError("masked vectors must be int32")
        if t.device != first.device or t.numel() != first.numel():
            raise ValueError("masked vectors differ in device or length")
    n = first.numel()
    secagg_ref.check_range(offset, n)
    if out is None:
        out = torch.empty(masked[survivors[0]].shape, dtype=out_dtype,
                          device=first.device)
    of = _flat(out, "out")
    if (of.dtype != out_dtype or of.device != first.device
            or of.numel() != n):
        raise ValueError(
            "out must match out_dtype and the masked vectors' device/length")

    if first.is_cuda:
        from rayfed_amd.ops import _hip_loader

        kt, st = _key_tensors(corr_keys, corr_signs)
        with torch.cuda.device(first.device):
            _hip_loader.load().secagg_aggregate_async(
                of, flats, kt, st, round, offset, frac_bits)
        return out
    res = secagg_ref.aggregate_ref(
        [t.numpy() for t in flats], corr_keys, corr_signs, round, offset,
        frac_bits, _DTYPE_NAMES[out_dtype])
    if out_dtype == torch.bfloat16:
        of.copy_(torch.from_numpy(res.view(np.int16)).view(torch.bfloat16))
    else:
        of.copy_(torch.from_numpy(res))
    return out
