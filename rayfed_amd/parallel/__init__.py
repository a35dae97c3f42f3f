"""Intra-party parallelism: RCCL-over-xGMI process groups and FedAvg
aggregation, plus pairwise-mask secure aggregation
across parties (``secagg``) with optional differential privacy (``dp``)."""
from rayfed_amd.parallel.dp import (  # noqa: F401
    BinomialNoise,
    clip_factor,
    sum_squares,
)
from rayfed_amd.parallel.secagg import (  # noqa: F401
    SecAggSession,
    aggregate,
    derive_pair_key,
)
