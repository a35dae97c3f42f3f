"""Secure aggregation end to end across three parties: each party masks a
seeded update in its own @fed.remote task, one party aggregates, and every
party checks the result against the quantised reference sum bit for bit."""
import numpy as np

import rayfed_amd as fed
from tests._util import run_parties

PARTIES = ("alice", "bob", "carol")
N = 1000
ROUND = 12
WEIGHTS = {"alice": 0.5, "bob": 0.25, "carol": 0.25}
SEEDS = {"alice": 1, "bob": 2, "carol": 3}


def _update(party):
    import torch

    g = torch.Generator().manual_seed(SEEDS[party])
    return torch.randn(N, generator=g)


def _driver_secagg(party, addresses):
    import torch

    from rayfed_amd.ops import secagg_ref
    from rayfed_amd.parallel import SecAggSession, aggregate

    fed.init(addresses=addresses, party=party, logging_level="warning")

    @fed.remote
    def masked_update(me):
        sess = SecAggSession.from_shared_secret(PARTIES, me, b"fed-test")
        return sess.mask(_update(me), round=ROUND, weight=WEIGHTS[me])

    @fed.remote
    def unmask(a, b, c):
        for y in (a, b, c):
            assert y.dtype == torch.int32 and y.shape == (N,)
        return aggregate({"alice": a, "bob": b, "carol": c}, PARTIES,
                         round=ROUND)

    ys = [masked_update.party(p).remote(p) for p in PARTIES]
    result = fed.get(unmask.party("carol").remote(*ys))

    acc = np.zeros(N, dtype=np.uint32)
    for p in PARTIES:
        acc += secagg_ref.quantize(_update(p).numpy(), WEIGHTS[p],
                                   16).view(np.uint32)
    want = acc.view(np.int32).astype(np.float32) * np.float32(2.0 ** -16)
    assert result.dtype == torch.float32
    assert np.array_equal(result.numpy(), want)
    fed.shutdown()


def test_secagg_three_parties_exact():
    run_parties(_driver_secagg, parties=PARTIES, timeout=120)
