"""Differentially private secure aggregation across three parties.

As examples/secure_agg.py, plus the two steps that make the *aggregate*
private as well: each party clips its update to an L2 bound
(``clip_factor`` — one read-only pass for the norm, folded into the weight)
and adds binomial noise (``BinomialNoise``) before masking.  The noise is an
exact integer function of a private ChaCha20 stream, generated inside the
same kernel that quantises and masks, so the result is still specified bit
for bit: the aggregate equals the ring sum of the clipped quantised updates
plus the three parties' reference noises, exactly (docs/secagg.md).

The noise keys are derived from fixed strings here so that the check below
can recompute them; a deployment uses ``BinomialNoise.fresh()`` and never
shares the key.  The pair keys come from one shared secret, a demo
convenience and not a key exchange.  One process per party; ``alice`` also
starts the third party as a child process:

    python examples/dp_secure_agg.py alice     # launches carol too
    python examples/dp_secure_agg.py bob

or start all three yourself with ``alice --no-spawn``, ``bob``, ``carol``.
"""
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rayfed_amd as fed
from rayfed_amd.ops import secagg_ref
from rayfed_amd.parallel import (
    BinomialNoise,
    SecAggSession,
    aggregate,
    clip_factor,
)

PARTIES = ("alice", "bob", "carol")
WEIGHTS = {"alice": 0.5, "bob": 0.3, "carol": 0.2}  # e.g. sample shares
SEEDS = {"alice": 1, "bob": 2, "carol": 3}
SCALES = {"alice": 0.5, "bob": 1.0, "carol": 2.0}  # carol's norm gets clipped
SECRET = b"demo-secret-provisioned-out-of-band"
N = 1 << 20
ROUND = 7
FRAC_BITS = 16
CLIP_NORM = 1200.0  # ||randn(N)|| is about 1024
WORDS, STEP = 4, 64  # per-party noise std = 64*sqrt(32)/2^16, about 5.5e-3


def local_update(party):
    g = torch.Generator(device="cpu").manual_seed(SEEDS[party])
    return torch.randn(N, generator=g) * SCALES[party]


def noise_of(party):
    return BinomialNoise(hashlib.sha256(b"demo-noise-" + party.encode())
                         .digest(), words=WORDS, step=STEP)


def main(party):
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    addresses = {"alice": "127.0.0.1:11042", "bob": "127.0.0.1:11041",
                 "carol": "127.0.0.1:11043"}
    fed.init(addresses=addresses, party=party)

    @fed.remote
    def masked_update(me):
        sess = SecAggSession.from_shared_secret(PARTIES, me, SECRET,
                                                FRAC_BITS)
        x = local_update(me).to(dev)
        w = WEIGHTS[me] * clip_factor(x, CLIP_NORM)
        return sess.mask(x, round=ROUND, weight=w, noise=noise_of(me)), w

    @fed.remote
    def unmask(a, b, c):
        masked = {"alice": a[0], "bob": b[0], "carol": c[0]}
        masked = {p: t.to(dev) for p, t in masked.items()}
        out = aggregate(masked, PARTIES, round=ROUND, frac_bits=FRAC_BITS)
        return out.cpu(), {"alice": a[1], "bob": b[1], "carol": c[1]}

    ys = [masked_update.party(p).remote(p) for p in PARTIES]
    result, used = fed.get(unmask.party("bob").remote(*ys))

    # Reference: quantised clipped updates plus the three reference noises,
    # summed in the ring and dequantised.  (The weights the parties report
    # are used as they are: the norm behind them is a float64 sum whose
    # last bits may depend on the device that computed it.)
    acc = np.zeros(N, dtype=np.uint32)
    for p in PARTIES:
        acc += secagg_ref.quantize(local_update(p).numpy(), used[p],
                                   FRAC_BITS).view(np.uint32)
        acc += secagg_ref.binomial_noise(noise_of(p).key, ROUND, 0, N, WORDS,
                                         STEP)
    expect = (acc.view(np.int32).astype(np.float32)
              * np.float32(2.0 ** -FRAC_BITS))
    assert np.array_equal(result.numpy(), expect), "aggregate is not exact"
    for p in PARTIES:
        c = clip_factor(local_update(p), CLIP_NORM)
        assert abs(used[p] - WEIGHTS[p] * c) <= 1e-9 * used[p], p
    assert used["carol"] < WEIGHTS["carol"], "carol should have been clipped"
    plain = sum(used[p] * local_update(p) for p in PARTIES)
    noise = noise_of(party)
    err = float((result - plain).abs().max())
    bound = noise.max_abs(FRAC_BITS, contributors=3) + 3.0 * 2.0 ** -FRAC_BITS
    assert err <= bound, (err, bound)
    print(f"[{party}] DP aggregate == quantised clipped sum + 3 reference "
          f"noises, bit for bit; noise std "
          f"{noise.std(FRAC_BITS, contributors=3):.2e} (measured "
          f"{float((result - plain).std()):.2e}), max |error| {err:.2e} <= "
          f"{bound:.2e}")
    fed.shutdown()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--no-spawn"]
    assert len(args) == 1 and args[0] in PARTIES, (
        "Please run this script with a party name: alice, bob or carol.")
    child = None
    if args[0] == "alice" and "--no-spawn" not in sys.argv:
        child = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "carol"])
    try:
        main(args[0])
        if child is not None:
            assert child.wait(timeout=60) == 0, "carol failed"
    finally:
        if child is not None and child.poll() is None:
            child.kill()
            child.wait()
