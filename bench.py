#!/usr/bin/env python3
"""Flagship benchmark — BASELINE.json headline metric on MI355X.

Metric: cross-party objects/sec of the many_tiny_tasks harness
(/root/reference/benchmarks/many_tiny_tasks_benchmark.py:44-59 — per
iteration: one actor task per party + one cross-party aggregate + one
fed.get broadcast → 2 cross-party object transfers), measured on this
engine's control path.

Scaling model (``--gpus N``, weak): N GPUs are split across the two parties
(alice = GPUs [0, N/2), bob = the rest).  Each GPU pair (i, i+N/2) runs one
federation *lane* — an independent 2-party fed job on its own loopback ports
— so per-GPU work is fixed while whole-job objects/sec grows with N.
N=1 runs both parties of one lane on GPU 0 (bob in a forked subprocess).

Launch contract (driver): ``python bench.py --gpus N --steps K --warmup W``;
for N>1 via ``python -m torch.distributed.run --nproc-per-node N`` — one
rank per GPU, rank r < N/2 drives alice of lane r, rank r >= N/2 drives bob
of lane r-N/2.  Rank 0 prints ONE JSON line; elapsed is the MAX over ranks.

Modes: ``tiny`` (headline; ``--parties 3 --tls`` for BASELINE config 5),
``push`` (config 3: 4 GiB bf16 tensor push alice→bob over the device-IPC
lane; ``RAYFED_BENCH_WIRE_FP8=1`` for fp8 wire; ``RAYFED_SHM=0`` for the
cross-host-shaped socket lane), ``fedavg`` (config 4: Llama-3-8B
gradients, intra-party RCCL + cross-party exchange + HIP combine;
``RAYFED_BENCH_ARENA=1`` for the zero-pack shared-gradient arena).

A plain run does only what its headline figure needs: set up, warm up,
time ``--steps`` steps, print the JSON line.  ``--full`` (tiny N=1 GPU run)
ALSO measures push / fedavg / arena-fedavg / socket-push / tls-push in
subprocesses and reports them under ``config.extras`` so a single
invocation observes every data-plane headline.  The JSON line always
carries ``transport`` (cpp/asyncio/grpc) and, for data modes, the ``lane``.

``--dump-outputs DIR`` writes what the last timed step returned to its
caller (the ``fed.get`` value of that step) as ``DIR/last_step_result.npy``
(float64).  Inputs are seeded, so two builds run with the same arguments
can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import sys
import time


def _has_cuda():
    try:
        import torch

        return torch.cuda.is_available()
    except ImportError:
        return False


def _transport_in_use() -> str:
    """Which cross-silo transport the running fed job selected (must be
    reported in the bench JSON — VERDICT r1: a driver run on the asyncio
    fallback must be distinguishable from the C++ lane)."""
    from rayfed_amd.proxy import barriers

    svc = barriers._sender_service
    if svc is None:
        return "none"
    name = type(svc).__name__
    if name == "XferSenderService":
        return "cpp"
    proxy = getattr(svc, "proxy", None)
    pname = type(proxy).__name__ if proxy is not None else ""
    if "Grpc" in pname:
        return "grpc"
    return "asyncio"


def _pin_cpus(rank: int = 0, world: int = 1):
    """Pin this process to a compact core set: 256-core boxes migrate the
    hot threads across CCDs otherwise (measured 0.34 -> 0.25 ms/round at
    the driver shape, 0.27 -> 0.18 warm, same box).  RAYFED_BENCH_AFFINITY=0
    disables.  Harness-level tuning only — the library never pins."""
    if os.environ.get("RAYFED_BENCH_AFFINITY", "1") == "0":
        return
    try:
        ncpu = os.cpu_count() or 1
        per = max(8, min(32, ncpu // max(1, world)))
        lo = min(rank * per, max(0, ncpu - per))
        os.sched_setaffinity(0, set(range(lo, min(ncpu, lo + per))))
    except (AttributeError, OSError, ValueError):
        pass


def _warm_transport(addresses, party, rounds: int = 32):
    """Pre-warm connections + receiver conn threads with readiness pings.
    Infrastructure-only warmup (no benchmark work): the driver's round uses
    W=5, far too few rounds to absorb connect/thread-spawn costs."""
    import socket

    from rayfed_amd._private import constants
    from rayfed_amd.proxy import barriers

    svc = barriers._sender_service
    others = [p for p in addresses if p != party]
    # Wait for every peer port to accept first — a ping against a
    # not-yet-listening receiver burns the transport's retry backoff.
    deadline = time.monotonic() + 60
    for other in others:
        host, port = addresses[other].rsplit(":", 1)
        while time.monotonic() < deadline:
            try:
                socket.create_connection((host, int(port)), timeout=1).close()
                break
            except OSError:
                time.sleep(0.05)
    for _ in range(rounds):
        for other in others:
            try:
                svc.send(
                    other, b"data", constants.PING_SEQ_ID, constants.PING_SEQ_ID
                ).result(timeout=10)
            except Exception:  # noqa: BLE001 — peer may still be starting
                time.sleep(0.05)


def _dump_outputs(dump_dir: str, result) -> None:
    """--dump-outputs: the value the last timed step handed its caller."""
    import numpy as np

    os.makedirs(dump_dir, exist_ok=True)
    arr = np.atleast_1d(np.asarray(result, dtype=np.float64))
    np.save(os.path.join(dump_dir, "last_step_result.npy"), arr)


# ------------------------------------------------------------------ tiny mode
def _tiny_driver(party: str, addresses, steps: int, warmup: int, device: int,
                 job_name: str, tls_config=None, barrier_cb=None, result_q=None,
                 dump_dir=None):
    """The many_tiny_tasks loop; identical code runs in every party."""
    import rayfed_amd as fed

    use_gpu = _has_cuda()
    if use_gpu:
        import torch

        torch.cuda.set_device(device)

    fed.init(addresses=addresses, party=party, job_name=job_name,
             tls_config=tls_config, logging_level="warning")
    parties = sorted(addresses)

    @fed.remote
    class MyActor:
        def __init__(self, device, use_gpu):
            self._use_gpu = use_gpu
            if use_gpu:
                import torch

                self._t = torch.zeros(256, device=f"cuda:{device}")

        def run(self):
            if self._use_gpu:
                self._t += 1.0  # a real (tiny) HIP kernel per task
            return 1

    @fed.remote
    class Aggregator:
        def aggr(self, *vals):
            return sum(vals)

    actors = [MyActor.party(p).remote(device, use_gpu) for p in parties]
    aggregator = Aggregator.party(parties[0]).remote()

    _warm_transport(addresses, party)
    transport = _transport_in_use()

    def one_iter():
        vals = [a.run.remote() for a in actors]
        s = aggregator.aggr.remote(*vals)
        return fed.get(s)

    for _ in range(warmup):
        assert one_iter() == len(parties)
    if use_gpu:
        import torch

        torch.cuda.synchronize()
    if barrier_cb is not None:
        barrier_cb()
    debug = os.environ.get("RAYFED_BENCH_DEBUG") == "1"
    stamps = [0.0] * (steps + 1) if debug else None
    last = None
    t0 = time.perf_counter()
    if debug:
        for i in range(steps):
            last = one_iter()
            stamps[i + 1] = time.perf_counter() - t0
    else:
        for _ in range(steps):
            last = one_iter()
    if use_gpu:
        import torch

        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if barrier_cb is not None:
        barrier_cb()
    if dump_dir is not None:
        _dump_outputs(dump_dir, last)
    if debug and party == sorted(addresses)[0]:
        per = [
            round((stamps[i + 1] - stamps[i]) * 1e6)
            for i in range(steps)
        ]
        print(f"[bench-debug] per-step us: {per}", file=sys.stderr)
    fed.shutdown()
    if result_q is not None:
        result_q.put((elapsed, transport))
    return elapsed, transport


# ------------------------------------------------------------------ push mode
_LANE_NAMES = {
    "ipc_group": "device-ipc",
    "ipc": "device-ipc",
    "shm_gpu": "shm-dma",
    "shm_chunked": "shm-dma",
    "shm_cpu": "shm-dma",
    "payload": "socket",
}


def _detect_lane(nbytes: int, dtype, device_type: str) -> str:
    """Name the lane (device-ipc / shm-dma / socket) a tensor of this shape
    rides on the current sender — reported in the bench JSON."""
    from rayfed_amd.ops import shm_pool, tensor_codec
    from rayfed_amd.proxy import barriers

    svc = barriers._sender_service
    plane = getattr(getattr(svc, "proxy", None), "gpu_plane", None)
    route = tensor_codec.route_for_spec(
        nbytes, dtype, device_type, plane, shm_pool.shm_enabled()
    )
    return _LANE_NAMES.get(route, route)


def _push_driver(party: str, addresses, steps: int, warmup: int, device: int,
                 job_name: str, nbytes: int, tls_config=None, barrier_cb=None,
                 result_q=None, dump_dir=None):
    """BASELINE config 3: bf16 tensor push alice→bob; end-to-end GB/s."""
    import torch

    import rayfed_amd as fed

    use_gpu = _has_cuda()
    dev = f"cuda:{device}" if use_gpu else "cpu"
    if use_gpu:
        torch.cuda.set_device(device)
    cfg = {}
    if os.environ.get("RAYFED_BENCH_WIRE_FP8") == "1":
        cfg["gpu_data_plane"] = {"wire_dtype": "fp8e4m3"}
    fed.init(addresses=addresses, party=party, job_name=job_name,
             config=cfg, tls_config=tls_config, logging_level="warning")

    numel = nbytes // 2

    @fed.remote
    class Producer:
        def __init__(self, dev, numel):
            torch.manual_seed(0)  # same payload run to run
            self._t = torch.randn(numel, dtype=torch.bfloat16, device=dev)

        def produce(self):
            return self._t

    @fed.remote
    class Consumer:
        def consume(self, t):
            return int(t.numel() * t.element_size())

    producer = Producer.party("alice").remote(dev, numel)
    consumer = Consumer.party("bob").remote()
    _warm_transport(addresses, party)
    transport = _transport_in_use()

    def one_iter():
        t = producer.produce.remote()
        n = consumer.consume.remote(t)
        return fed.get(n)

    for _ in range(warmup):
        assert one_iter() == nbytes
    if use_gpu:
        torch.cuda.synchronize()
    if barrier_cb is not None:
        barrier_cb()
    last = None
    t0 = time.perf_counter()
    for _ in range(steps):
        last = one_iter()
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if barrier_cb is not None:
        barrier_cb()
    if dump_dir is not None:
        _dump_outputs(dump_dir, last)
    lane = "n/a"
    if party == "alice":
        try:
            lane = _detect_lane(nbytes, torch.bfloat16, "cuda" if use_gpu else "cpu")
        except Exception:  # noqa: BLE001
            lane = "unknown"
    fed.shutdown()
    if result_q is not None:
        result_q.put((elapsed, transport, lane))
    return elapsed, transport, lane


# ---------------------------------------------------------------- fedavg mode
def llama3_8b_grad_shapes(layers: int = 32, vocab: int = 128256):
    """Parameter shapes of Llama-3-8B (vocab 128256, d=4096, ffn 14336,
    32 layers, GQA kv 1024) — synthetic gradients of this architecture.
    ``vocab`` shrinks the embedding for small smoke runs only."""
    shapes = [(vocab, 4096)]  # embed
    for _ in range(layers):
        shapes += [
            (4096, 4096),   # q
            (1024, 4096),   # k
            (1024, 4096),   # v
            (4096, 4096),   # o
            (14336, 4096),  # gate
            (14336, 4096),  # up
            (4096, 14336),  # down
            (4096,), (4096,),  # norms
        ]
    shapes += [(4096,), (vocab, 4096)]  # final norm, lm_head
    return shapes


def _fedavg_driver(party, addresses, steps, warmup, device, job_name, layers,
                   vocab=128256, party_group=None, barrier_cb=None,
                   result_q=None, dump_dir=None):
    """Party-leader FedAvg round: (optional) intra-party RCCL all-reduce,
    cross-party gradient exchange through the fed data plane, HIP weighted
    combine (csrc fedavg_reduce_)."""
    import torch

    import rayfed_amd as fed
    from rayfed_amd.parallel.fedavg import weighted_combine_

    use_gpu = _has_cuda()
    dev = f"cuda:{device}" if use_gpu else "cpu"
    if use_gpu:
        torch.cuda.set_device(device)
    # Zero-copy receive: the combine reads the peer's IPC slabs directly
    # (fused combine+verify kernel) instead of materializing a copy.
    fed.init(addresses=addresses, party=party, job_name=job_name,
             config={"gpu_data_plane": {"lazy_ipc": True}},
             logging_level="warning")

    dtype = torch.bfloat16
    torch.manual_seed(0 if party == "alice" else 1)
    # Flat gradient buffer with per-parameter VIEWS (the flat-grads layout
    # production DDP keeps): the cross-party push and the intra-party
    # all-reduce both operate on `flat` directly — no per-round repack.
    # RAYFED_BENCH_ARENA=1: the gradients LIVE in IPC-shared arena slabs
    # instead — the exchange ships (handle, hash) per shard, zero pack.
    shapes = llama3_8b_grad_shapes(layers, vocab)
    total = sum(int(torch.prod(torch.tensor(sh))) for sh in shapes)
    # Arena mode is a single-node N=1 measurement variant: torchrun member
    # ranks mirror the flat-buffer collective, so leaders must match.
    use_arena = (
        os.environ.get("RAYFED_BENCH_ARENA") == "1"
        and use_gpu
        and os.environ.get("WORLD_SIZE", "1") == "1"
    )
    if use_arena:
        from rayfed_amd.ops.gpu_plane import maybe_create_gpu_plane

        plane = maybe_create_gpu_plane({"lazy_ipc": True})
        arena = plane.alloc_shared_arena(total * 2)
        S = arena.SLAB // 2  # bf16 elements per slab
        shards = []
        left = total
        for sv in arena.shards:
            n_el = min(left, sv.numel() // 2)
            if n_el <= 0:
                break
            shards.append(sv[: n_el * 2].view(dtype))
            left -= n_el
        flat = None
        for sh in shards:
            sh.uniform_(-1, 1)
    else:
        flat = torch.empty(total, dtype=dtype, device=dev).uniform_(-1, 1)
        shards = None
    nbytes = total * 2
    from rayfed_amd.parallel.fedavg import allreduce_flat_

    @fed.remote
    class Exchanger:
        """Receives the peer's averaged grads and combines with local."""

        def combine(self, peer_flat, local_flat):
            if isinstance(local_flat, (list, tuple)):  # arena shards
                acc = 0.0
                for pv, lv in zip(peer_flat, local_flat):
                    out = torch.empty_like(lv)
                    weighted_combine_(out, [lv, pv], [0.5, 0.5])
                    acc += float(out[:2].float().sum())
                torch.cuda.synchronize()
                return acc
            out = torch.empty_like(local_flat)
            weighted_combine_(out, [local_flat, peer_flat], [0.5, 0.5])
            if out.is_cuda:
                torch.cuda.synchronize()
            return float(out[:2].float().sum())

    exchangers = {
        "alice": Exchanger.party("alice").remote(),
        "bob": Exchanger.party("bob").remote(),
    }
    _warm_transport(addresses, party)
    transport = _transport_in_use()
    @fed.remote
    def produce(_tick):
        if party_group is not None:
            # Intra-party RCCL over xGMI, in place on the flat buffer.
            if shards is not None:
                for sh in shards:
                    allreduce_flat_(sh, group=party_group)
            else:
                allreduce_flat_(flat, group=party_group)
        return shards if shards is not None else flat

    def round_once(tick):
        fa = produce.party("alice").remote(tick)
        fb = produce.party("bob").remote(tick)
        ca = exchangers["alice"].combine.remote(fb, fa)
        cb = exchangers["bob"].combine.remote(fa, fb)
        return fed.get([ca, cb])

    for i in range(warmup):
        round_once(("w", i))
    if use_gpu:
        torch.cuda.synchronize()
    if barrier_cb is not None:
        barrier_cb()
    last = None
    t0 = time.perf_counter()
    for i in range(steps):
        last = round_once(("s", i))
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if barrier_cb is not None:
        barrier_cb()
    if dump_dir is not None:
        _dump_outputs(dump_dir, last)
    try:
        lane = _detect_lane(nbytes, dtype, "cuda" if use_gpu else "cpu")
    except Exception:  # noqa: BLE001
        lane = "unknown"
    fed.shutdown()
    if result_q is not None:
        result_q.put((elapsed, nbytes, transport, lane))
    return elapsed, nbytes, transport, lane


_DRIVERS = {"tiny": _tiny_driver, "push": _push_driver, "fedavg": _fedavg_driver}


def _run_fedavg_torchrun(steps, warmup, layers, vocab, rank, world, local_rank,
                         dump_dir=None):
    """Leaders (ranks 0, W/2) run the fed exchange; every rank joins its
    party's RCCL group for the intra-party gradient all-reduce."""
    import torch
    import torch.distributed as dist

    _pin_cpus(local_rank, world)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    half = world // 2
    party = "alice" if rank < half else "bob"
    use_gpu = _has_cuda()
    backend = "nccl" if use_gpu else "gloo"
    if use_gpu:
        # Modulo device_count: a no-op on the 8-GPU node; lets the torchrun
        # path run (ranks sharing GPU 0) on 1-GPU validation boxes.
        local_rank = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
    alice_g = dist.new_group(list(range(half)), backend=backend)
    bob_g = dist.new_group(list(range(half, world)), backend=backend)
    group = alice_g if party == "alice" else bob_g
    is_leader = rank in (0, half)
    base = int(os.environ.get("RAYFED_BENCH_BASE_PORT", "23500"))
    addresses = {
        "alice": f"127.0.0.1:{base}",
        "bob": f"127.0.0.1:{base + 1}",
    }

    def barrier():
        dist.barrier()

    transport, lane = "n/a", "n/a"
    if is_leader and half >= 1:
        elapsed, nbytes, transport, lane = _fedavg_driver(
            party, addresses, steps, warmup, local_rank, "bench_fedavg", layers,
            vocab=vocab, party_group=group if half > 1 else None,
            barrier_cb=barrier, dump_dir=dump_dir if rank == 0 else None,
        )
    else:
        # Member rank: mirror the leader's per-round intra-party all-reduce.
        from rayfed_amd.parallel.fedavg import allreduce_flat_

        dev = f"cuda:{local_rank}" if use_gpu else "cpu"
        torch.manual_seed(rank)
        shapes = llama3_8b_grad_shapes(layers, vocab)
        total = sum(int(torch.prod(torch.tensor(sh))) for sh in shapes)
        flat = torch.empty(total, dtype=torch.bfloat16, device=dev).uniform_(-1, 1)
        nbytes = total * 2
        for _ in range(warmup):
            allreduce_flat_(flat, group=group)
        if use_gpu:
            torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            allreduce_flat_(flat, group=group)
        if use_gpu:
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        barrier()
    t = __import__("torch").tensor([elapsed], dtype=__import__("torch").float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.destroy_process_group()
    return float(t.item()), nbytes, transport, lane


def _run_single_process(mode, steps, warmup, extra=None, parties=2, tls=False,
                        dump_dir=None):
    """N=1: first party in-process, the rest forked, all on GPU 0."""
    _pin_cpus(0, 1)  # forked parties inherit the affinity set
    from tests._util import make_addresses  # free-port helper

    names = ["alice", "bob", "carol", "dave"][:parties]
    addresses = make_addresses(names)
    ctx = multiprocessing.get_context("fork")
    tls_config = None
    if tls:
        import sys as _sys

        _sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from tool.generate_tls_certs import generate

        tls_config = generate("/tmp/rayfed_amd/bench-certs")
        tls_config["target_name_override"] = "localhost"
    if mode == "fedavg":
        args_extra = tuple(extra)  # (layers, vocab)
    elif mode == "push":
        args_extra = (extra, tls_config)
    else:
        args_extra = (tls_config,)
    procs = [
        ctx.Process(
            target=_DRIVERS[mode],
            args=(name, addresses, steps, warmup, 0, f"bench_{mode}") + args_extra,
            daemon=True,  # die with the driver — never orphan a party
        )
        for name in names[1:]
    ]
    for p in procs:
        p.start()
    elapsed = _DRIVERS[mode](
        names[0], addresses, steps, warmup, 0, f"bench_{mode}", *args_extra,
        dump_dir=dump_dir,
    )
    for p in procs:
        p.join(timeout=600)
        if p.is_alive():
            p.terminate()
            raise RuntimeError("peer party hung")
    return elapsed


def _run_torchrun(mode, steps, warmup, push_bytes, rank, world, local_rank,
                  dump_dir=None):
    import torch.distributed as dist

    _pin_cpus(local_rank, world)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    if _has_cuda():
        import torch

        # No-op on the 8-GPU node; lets 1-GPU boxes validate this path.
        local_rank = local_rank % torch.cuda.device_count()
    lanes = world // 2
    lane = rank % lanes
    party = "alice" if rank < lanes else "bob"
    base = int(os.environ.get("RAYFED_BENCH_BASE_PORT", "23500"))
    addresses = {
        "alice": f"127.0.0.1:{base + lane * 2}",
        "bob": f"127.0.0.1:{base + lane * 2 + 1}",
    }

    def barrier():
        dist.barrier()

    args_extra = (push_bytes,) if mode == "push" else ()
    out = _DRIVERS[mode](
        party, addresses, steps, warmup, local_rank, f"bench_{mode}_lane{lane}",
        *args_extra, barrier_cb=barrier,
        dump_dir=dump_dir if rank == 0 else None,
    )
    if mode == "push":
        elapsed, transport, data_lane = out
    else:  # tiny
        elapsed, transport = out
        data_lane = "n/a"
    # MAX over ranks (the contract).
    import torch

    t = torch.tensor([elapsed], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.destroy_process_group()
    return float(t.item()), lanes, transport, data_lane


def _run_extras() -> dict:
    """--full: measure BASELINE configs 3 (4 GiB push) and 4 (FedAvg) in
    fresh subprocesses so one run observes the data-plane numbers too.
    Failures degrade to an error note, never crash the headline run."""
    import subprocess

    out = {}
    specs = [
        ("push", ["--mode", "push", "--steps", "8", "--warmup", "2"], 360, {}),
        ("fedavg", ["--mode", "fedavg", "--steps", "5", "--warmup", "1"], 360,
         {}),
        # Zero-pack variant: gradients live in a persistent IPC-shared
        # arena; the exchange ships (slab handle, hash) per shard.
        ("fedavg_arena",
         ["--mode", "fedavg", "--steps", "5", "--warmup", "1"], 360,
         {"RAYFED_BENCH_ARENA": "1"}),
        # Cross-host-shaped lane: same push with the same-host fast lanes
        # disabled, so the striped/chunk-streamed socket path is measured.
        ("socket_push",
         ["--mode", "push", "--steps", "4", "--warmup", "1",
          "--push-gib", "2"], 360, {"RAYFED_SHM": "0"}),
        # Same shape under mutual TLS: the chunk-streamed path rides striped
        # parallel TLS connections (crypto parallelizes with assembly).
        ("tls_push",
         ["--mode", "push", "--steps", "4", "--warmup", "1",
          "--push-gib", "2", "--tls"], 360, {"RAYFED_SHM": "0"}),
    ]
    env = dict(os.environ)
    for name, flags, tmo, extra_env in specs:
        try:
            r = subprocess.run(
                [sys.executable, os.path.abspath(__file__)] + flags,
                capture_output=True, text=True, timeout=tmo,
                env={**env, **extra_env},
                cwd=os.path.dirname(os.path.abspath(__file__)),
            )
            line = next(
                ln for ln in reversed(r.stdout.strip().splitlines())
                if ln.startswith("{")
            )
            j = json.loads(line)
            out[f"{name}_GBps"] = j["value"]
            out[f"{name}_ms_per_step"] = j["ms_per_step"]
            out[f"{name}_lane"] = j["config"].get("lane")
            out[f"{name}_transport"] = j.get("transport")
        except Exception as e:  # noqa: BLE001
            out[f"{name}_error"] = repr(e)[:300]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=None,
                   help="timed steps (default: 2000 tiny, 10 push/fedavg)")
    p.add_argument("--warmup", type=int, default=None,
                   help="untimed steps (default: 200 tiny, 2 push/fedavg)")
    p.add_argument("--mode", choices=["tiny", "push", "fedavg"], default="tiny")
    p.add_argument("--push-gib", type=float, default=4.0,
                   help="tensor size for --mode push (GiB)")
    p.add_argument("--layers", type=int, default=32,
                   help="transformer layers for --mode fedavg (32 = Llama-3-8B)")
    p.add_argument("--vocab", type=int, default=128256,
                   help="embedding vocab for --mode fedavg (smoke runs only)")
    p.add_argument("--parties", type=int, default=2,
                   help="party count for --mode tiny at N=1 (config 5 uses 3)")
    p.add_argument("--tls", action="store_true",
                   help="self-signed mutual TLS on the cross-silo link")
    p.add_argument("--full", action="store_true",
                   help="also measure push / fedavg / socket / TLS lanes in "
                        "subprocesses (config.extras); tiny N=1 GPU run only")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's result to "
                        "DIR/last_step_result.npy")
    args = p.parse_args()

    # GiB-scale payload per step in the data modes: their DEFAULT run stays
    # under minutes.  An explicit --steps / --warmup is always honoured.
    heavy = args.mode in ("push", "fedavg")
    if args.steps is None:
        args.steps = 10 if heavy else 2000
    if args.warmup is None:
        args.warmup = 2 if heavy else 200
    if args.steps < 1:
        p.error("--steps must be >= 1")
    push_bytes = (int(args.push_gib * (1 << 30)) // 2) * 2  # whole bf16 elements

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    fedavg_nbytes = None
    transport, data_lane = "n/a", "n/a"
    if world > 1:
        assert world % 2 == 0, "world size must be even (2 parties)"
        if args.mode == "fedavg":
            elapsed, fedavg_nbytes, transport, data_lane = _run_fedavg_torchrun(
                args.steps, args.warmup, args.layers, args.vocab, rank, world,
                local_rank, dump_dir=args.dump_outputs,
            )
            lanes = 1
        else:
            elapsed, lanes, transport, data_lane = _run_torchrun(
                args.mode, args.steps, args.warmup, push_bytes, rank, world,
                local_rank, dump_dir=args.dump_outputs,
            )
        if rank != 0:
            return
        n_gpus = world
    else:
        out = _run_single_process(
            args.mode, args.steps, args.warmup,
            (args.layers, args.vocab) if args.mode == "fedavg" else push_bytes,
            parties=args.parties if args.mode == "tiny" else 2,
            tls=args.tls, dump_dir=args.dump_outputs,
        )
        if args.mode == "fedavg":
            elapsed, fedavg_nbytes, transport, data_lane = out
        elif args.mode == "push":
            elapsed, transport, data_lane = out
        else:
            elapsed, transport = out
        lanes, n_gpus = 1, args.gpus

    ms_per_step = elapsed * 1000.0 / args.steps
    n_parties = args.parties if (args.mode == "tiny" and world <= 1) else 2
    if args.mode == "fedavg":
        # Gradient bytes exchanged cross-party per round (both directions).
        value = 2.0 * fedavg_nbytes * args.steps / elapsed / 1e9
        metric = "fedavg_cross_party_GBps"
        unit = "GB/s"
        config = {
            "model": f"Llama-3-8B synthetic gradients ({args.layers} layers)",
            "global_batch": args.steps,
            "seq_len": fedavg_nbytes // 2,
            "parallelism": f"2 parties x {max(1, world // 2)} GPUs, RCCL intra-party",
            "grad_gib": round(fedavg_nbytes / (1 << 30), 2),
        }
    elif args.mode == "tiny":
        # Per iteration per lane: (P-1) value pushes into the aggregator's
        # party + (P-1) result broadcasts on fed.get.
        transfers = 2 * (n_parties - 1)
        value = float(transfers) * args.steps * lanes / elapsed
        metric = "cross_party_objects_per_sec"
        unit = "objects/s"
        config = {
            "model": f"many_tiny_tasks ({n_parties}-party aggregate loop"
                     + (", TLS" if args.tls else "") + ")",
            "global_batch": args.steps * lanes,
            "seq_len": 1,
            "parallelism": f"fed2p-weak x{lanes} lanes",
            "per_task_overhead_ms": ms_per_step,
        }
    else:
        value = push_bytes * args.steps * lanes / elapsed / 1e9
        metric = "cross_party_tensor_push_GBps"
        unit = "GB/s"
        config = {
            "model": f"{args.push_gib} GiB bf16 tensor push alice->bob"
                     + (", TLS" if args.tls else ""),
            "global_batch": args.steps,
            "seq_len": push_bytes // 2,
            "parallelism": f"fed2p-weak x{lanes} lanes",
        }

    # Honest labeling: tiny-mode payloads are Python ints — the
    # reference benchmark's exact object shape — not bf16 tensors.
    dtype = "int64" if args.mode == "tiny" else "bf16"
    config["transport"] = transport
    if args.mode != "tiny":
        config["lane"] = data_lane

    # --full on the (tiny, N=1, GPU) run also measures the 4 GiB push and
    # the FedAvg round in subprocesses — outside the timed region, reported
    # alongside the headline metric.
    if (
        args.full
        and args.mode == "tiny"
        and world <= 1
        and not args.tls
        and _has_cuda()
    ):
        config["extras"] = _run_extras()

    print(json.dumps({
        "metric": metric,
        "value": round(value, 3),
        "unit": unit,
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype,
        "data": "synthetic",
        "transport": transport,
        "config": config,
    }))


if __name__ == "__main__":
    main()
