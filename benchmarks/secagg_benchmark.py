"""Secure-aggregation kernel benchmark (single GPU, standalone).

Times, with device events around each call after a warm-up:

  * ``secagg_mask_async`` for 1, 3 and 7 peers on bf16 and fp32 input;
  * ``secagg_aggregate_async`` for K in {2, 4, 8} inputs with C in {0, 4}
    dropout corrections;
  * ``fedavg_reduce_`` fp32 at the same K and n in the same process — the
    yardstick: ``aggregate`` with C = 0 has the same access pattern (K
    16-byte loads and one 16-byte store per lane) and less arithmetic.
    The two are timed alternately, call by call, so drift hits both.

Then the differential-privacy kernels (``--sections dp`` runs only these):

  * ``secagg_mask_noise_async`` at W = 4 words per element for 1, 3 and 7
    peers on bf16 and fp32 input, each against the yardstick
    ``secagg_mask_async`` at ``peers + 4`` (the same number of ChaCha20
    blocks per 16 elements), interleaved call by call;
  * ``sumsq_async`` on bf16 and fp32 against ``hash64_async`` over the same
    bytes — the project's read-only streaming pass.

Bytes are the compulsory traffic computed from the shapes (inputs read once,
output written once).  One JSON line per configuration, then the
aggregate/fedavg bandwidth ratio per K with the repeat-to-repeat spread; the
DP rows carry their time ratio against the yardstick and both spreads.

    python benchmarks/secagg_benchmark.py [--n 67108864] [--warmup 5]
                                          [--repeats 50]
                                          [--sections all|secagg|dp]

The default n (64 Mi elements: 256 MiB per fp32/int32 tensor) is past the
4 MiB L2 and, for every multi-tensor configuration, the 256 MiB Infinity
Cache.  A missing GPU or extension is an error — there is no CPU fallback.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUND = 17
FRAC_BITS = 16


def _keys(count):
    raw = b"".join(hashlib.sha256(b"bench-%d" % i).digest()
                   for i in range(count))
    kt = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy())
    signs = torch.tensor([1 if i % 2 == 0 else -1 for i in range(count)],
                         dtype=torch.int32)
    return kt.reshape(count, 32), signs


def _time_calls(fns, warmup, repeats):
    """Time each callable in ``fns`` ``repeats`` times, interleaved
    (a, b, a, b, ...); returns one list of milliseconds per callable."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[i].append(start.elapsed_time(stop))
    return times


def _stats(ms, nbytes):
    med = statistics.median(ms)
    return {
        "ms_median": round(med, 4),
        "ms_min": round(min(ms), 4),
        "ms_max": round(max(ms), 4),
        "gbps_median": round(nbytes / med / 1e6, 1),
        "gbps_best": round(nbytes / min(ms) / 1e6, 1),
        "gbps_worst": round(nbytes / max(ms) / 1e6, 1),
    }


def _ratio(name, extra, t_new, t_ref):
    """Time ratio new/yardstick (> 1: the new kernel is slower), per-pair
    range, and the fastest-to-slowest spread of each side's repeats."""
    per_pair = [a / b for a, b in zip(t_new, t_ref)]
    rec = {"op": name}
    rec.update(extra)
    rec.update({
        "time_ratio_median": round(
            statistics.median(t_new) / statistics.median(t_ref), 4),
        "time_ratio_pairs_min": round(min(per_pair), 4),
        "time_ratio_pairs_max": round(max(per_pair), 4),
        "yardstick_spread": round(max(t_ref) / min(t_ref) - 1.0, 4),
        "new_spread": round(max(t_new) / min(t_new) - 1.0, 4),
    })
    return rec


def _dp_section(ext, n, dev, args):
    words = 4
    noise_key = torch.from_numpy(np.frombuffer(
        hashlib.sha256(b"bench-noise").digest(), dtype=np.uint8).copy())
    out_a = torch.empty(n, dtype=torch.int32, device=dev)
    out_b = torch.empty(n, dtype=torch.int32, device=dev)
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        x = torch.randn(n, device=dev).to(dtype)
        nbytes = n * (x.element_size() + 4)
        for peers in (1, 3, 7):
            kt, st = _keys(peers)
            ky, sy = _keys(peers + words)
            t_noise, t_mask = _time_calls(
                [lambda: ext.secagg_mask_noise_async(
                    x, out_a, kt, st, noise_key, words, 1000, ROUND, 0, 1.0,
                    FRAC_BITS),
                 lambda: ext.secagg_mask_async(x, out_b, ky, sy, ROUND, 0,
                                               1.0, FRAC_BITS)],
                args.warmup, args.repeats)
            rec = {"op": "mask+noise", "dtype": name, "peers": peers,
                   "words": words, "bytes": nbytes}
            rec.update(_stats(t_noise, nbytes))
            rec["gelem_per_s"] = round(
                n / statistics.median(t_noise) / 1e6, 2)
            print(json.dumps(rec), flush=True)
            rec = {"op": "mask", "dtype": name, "peers": peers + words,
                   "bytes": nbytes, "yardstick_for": "mask+noise"}
            rec.update(_stats(t_mask, nbytes))
            print(json.dumps(rec), flush=True)
            print(json.dumps(_ratio(
                "mask+noise_over_mask_at_peers_plus_words",
                {"dtype": name, "peers": peers, "words": words},
                t_noise, t_mask)), flush=True)
        nbytes = n * x.element_size()
        xb = x.view(torch.uint8)
        t_sq, t_hash = _time_calls(
            [lambda: ext.sumsq_async(x), lambda: ext.hash64_async(xb)],
            args.warmup, args.repeats)
        for op, ms in (("sumsq", t_sq), ("hash64", t_hash)):
            rec = {"op": op, "dtype": name, "bytes": nbytes}
            rec.update(_stats(ms, nbytes))
            print(json.dumps(rec), flush=True)
        print(json.dumps(_ratio("sumsq_over_hash64", {"dtype": name},
                                t_sq, t_hash)), flush=True)
        del x, xb


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1 << 26, help="elements")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--sections", choices=("all", "secagg", "dp"),
                    default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("secagg_benchmark needs a GPU")
    from rayfed_amd.ops import _hip_loader

    ext = _hip_loader.load()
    n = args.n
    dev = "cuda:0"
    print(json.dumps({"bench": "secagg", "n": n, "warmup": args.warmup,
                      "repeats": args.repeats,
                      "device": torch.cuda.get_device_name(0)}))

    if args.sections != "dp":
        _secagg_section(ext, n, dev, args)
    if args.sections != "secagg":
        _dp_section(ext, n, dev, args)


def _secagg_section(ext, n, dev, args):
    # ---- mask ------------------------------------------------------------
    out_i32 = torch.empty(n, dtype=torch.int32, device=dev)
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        x = torch.randn(n, device=dev).to(dtype)
        for peers in (1, 3, 7):
            kt, st = _keys(peers)
            (ms,) = _time_calls(
                [lambda: ext.secagg_mask_async(x, out_i32, kt, st, ROUND, 0,
                                               1.0, FRAC_BITS)],
                args.warmup, args.repeats)
            nbytes = n * (x.element_size() + 4)
            rec = {"op": "mask", "dtype": name, "peers": peers,
                   "bytes": nbytes}
            rec.update(_stats(ms, nbytes))
            med = statistics.median(ms)
            rec["gelem_per_s"] = round(n / med / 1e6, 2)
            rec["gmaskwords_per_s"] = round(n * peers / med / 1e6, 2)
            print(json.dumps(rec), flush=True)
        del x

    # ---- aggregate vs fedavg_reduce_ ------------------------------------
    ratios = {}
    for K in (2, 4, 8):
        ins_i = [torch.randint(-(2 ** 31), 2 ** 31 - 1, (n,),
                               dtype=torch.int32, device=dev)
                 for _ in range(K)]
        ins_f = [torch.randn(n, device=dev) for _ in range(K)]
        out_f = torch.empty(n, dtype=torch.float32, device=dev)
        out_y = torch.empty(n, dtype=torch.float32, device=dev)
        nbytes = n * 4 * (K + 1)
        k0, s0 = _keys(0)
        w = [1.0 / K] * K
        t_agg, t_fed = _time_calls(
            [lambda: ext.secagg_aggregate_async(out_f, ins_i, k0, s0, ROUND,
                                                0, FRAC_BITS),
             lambda: ext.fedavg_reduce_(out_y, ins_f, w)],
            args.warmup, args.repeats)
        for op, ms in (("aggregate", t_agg), ("fedavg_reduce_fp32", t_fed)):
            rec = {"op": op, "K": K, "C": 0, "bytes": nbytes}
            rec.update(_stats(ms, nbytes))
            print(json.dumps(rec), flush=True)
        per_pair = [f / a for a, f in zip(t_agg, t_fed)]  # >1: agg faster
        ratios[K] = {
            "K": K,
            "bw_ratio_median": round(
                statistics.median(t_fed) / statistics.median(t_agg), 4),
            "bw_ratio_pairs_min": round(min(per_pair), 4),
            "bw_ratio_pairs_max": round(max(per_pair), 4),
            "fedavg_spread": round(max(t_fed) / min(t_fed) - 1.0, 4),
            "aggregate_spread": round(max(t_agg) / min(t_agg) - 1.0, 4),
        }
        kc, sc = _keys(4)
        (ms,) = _time_calls(
            [lambda: ext.secagg_aggregate_async(out_f, ins_i, kc, sc, ROUND,
                                                0, FRAC_BITS)],
            args.warmup, args.repeats)
        rec = {"op": "aggregate", "K": K, "C": 4, "bytes": nbytes}
        rec.update(_stats(ms, nbytes))
        rec["gmaskwords_per_s"] = round(
            n * 4 / statistics.median(ms) / 1e6, 2)
        print(json.dumps(rec), flush=True)
        del ins_i, ins_f, out_f, out_y
    for K in (2, 4, 8):
        rec = {"op": "aggregate_C0_over_fedavg_reduce_fp32"}
        rec.update(ratios[K])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
