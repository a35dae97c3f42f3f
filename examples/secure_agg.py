"""Pairwise-mask secure aggregation across three parties.

Each party quantises its weighted update to fixed point in the ring Z/2^32
and adds one ChaCha20 keystream per peer, expanded on the device from the
pair's key (opposite signs at the two ends of a pair).  What travels is a
uniformly-masked int32 vector; the masks cancel **bit-exactly** in the ring
sum, so the aggregating party learns only the weighted aggregate.  Masking
and unmasking run as HIP kernels when a GPU is visible, and as the numpy
reference otherwise — both give identical bits (docs/secagg.md).

The pair keys here come from one shared secret, which is a demo
convenience and not a key exchange.  One process per party; to keep the
demo a two-terminal affair, ``alice`` also starts the third party as a
child process:

    python examples/secure_agg.py alice     # launches carol too
    python examples/secure_agg.py bob

or start all three yourself with ``alice --no-spawn``, ``bob``, ``carol``.
"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rayfed_amd as fed
from rayfed_amd.ops import secagg_ref
from rayfed_amd.parallel import SecAggSession, aggregate

PARTIES = ("alice", "bob", "carol")
WEIGHTS = {"alice": 0.5, "bob": 0.3, "carol": 0.2}  # e.g. sample shares
SEEDS = {"alice": 1, "bob": 2, "carol": 3}
SECRET = b"demo-secret-provisioned-out-of-band"
N = 1 << 20
ROUND = 7


def local_update(party):
    g = torch.Generator(device="cpu").manual_seed(SEEDS[party])
    return torch.randn(N, generator=g)


def main(party):
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    addresses = {"alice": "127.0.0.1:11032", "bob": "127.0.0.1:11031",
                 "carol": "127.0.0.1:11033"}
    fed.init(addresses=addresses, party=party)

    @fed.remote
    def masked_update(me):
        sess = SecAggSession.from_shared_secret(PARTIES, me, SECRET)
        return sess.mask(local_update(me).to(dev), round=ROUND,
                         weight=WEIGHTS[me])

    @fed.remote
    def unmask(a, b, c):
        masked = {"alice": a, "bob": b, "carol": c}
        masked = {p: t.to(dev) for p, t in masked.items()}
        return aggregate(masked, PARTIES, round=ROUND).cpu()

    ys = [masked_update.party(p).remote(p) for p in PARTIES]
    result = fed.get(unmask.party("bob").remote(*ys))

    # Reference: the ring sum of the UNMASKED quantised updates, dequantised.
    acc = np.zeros(N, dtype=np.uint32)
    for p in PARTIES:
        acc += secagg_ref.quantize(local_update(p).numpy(), WEIGHTS[p],
                                   16).view(np.uint32)
    expect = acc.view(np.int32).astype(np.float32) * np.float32(2.0 ** -16)
    assert np.array_equal(result.numpy(), expect), "masks did not cancel"
    plain = sum(WEIGHTS[p] * local_update(p) for p in PARTIES)
    err = float((result - plain).abs().max())
    print(f"[{party}] masked aggregate mean {float(result.mean()):.6f} == "
          f"quantised reference sum, bit for bit; max |error| vs the float "
          f"weighted sum {err:.2e} (fixed-point step {2.0 ** -16:.2e})")
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
