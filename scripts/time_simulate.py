#!/usr/bin/env python
"""Time the device simulator (pu_simulate_device) beside the host generator it relieves
(synthetic.simulate_states) on the benchmark shapes.

    python scripts/time_simulate.py [--out profiles/simulate_times.json] [--shapes cfg2 cfg3 cfg4]

Per shape: 3 warm-up calls, then 20 pu_simulate_device calls each between two HIP events on the
context's stream (the cumulative-row launch and the walk, tips only); the median is reported
with the minimum and maximum.  The host figure is the wall time of one
synthetic.simulate_states call on the same tree, model and number of sites.  The result is one
JSON document; DESIGN 4.10 quotes it.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {
    "cfg2": dict(subst="GTR+G4", alpha=0.5, ntax=50, sites=100_000),
    "cfg3": dict(subst="LG+G4", alpha=0.8, ntax=200, sites=10_000),
    "cfg4": dict(subst="GTR+G4", alpha=0.5, ntax=1000, sites=125_000),  # one device's shard
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host generator")
    args = ap.parse_args(argv)

    import torch

    from phylo_utils_amd import TreeModel, _native as N
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd import synthetic
    from phylo_utils_amd.rate_models import GammaRateModel

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    result = dict(arch=torch.cuda.get_device_properties(dev).gcnArchName, reps=args.reps,
                  warmup=args.warmup, shapes={})
    for name in args.shapes:
        cfg = SHAPES[name]
        model = SM.LG() if cfg["subst"].startswith("LG") else \
            SM.GTR(synthetic.CFG2_GTR_RATES, synthetic.CFG2_FREQS)
        rm = GammaRateModel(4, cfg["alpha"])
        tree = synthetic.random_tree(np.random.default_rng(0), cfg["ntax"])
        S, K = cfg["sites"], len(model.freqs)
        tm = TreeModel(keep_partials=False)
        tm.set_tree(tree)
        names = list(tm.traversal.names)
        tm.set_alignment_codes(np.zeros((len(names), 1), dtype=np.uint8), np.ones((1, K)), names)
        tm.set_substitution_model(model)
        tm.set_rate_model(rm)
        tm.initialise()
        N.check(N.lib().pu_ctx_set_stream(tm._ctx, ctypes.c_void_p(stream.cuda_stream)), tm._ctx)
        d_tips = torch.empty((len(names), S), dtype=torch.uint8, device=dev)

        def call(seed):
            N.check(N.lib().pu_simulate_device(tm._ctx, seed, 0, S,
                                               ctypes.c_void_p(d_tips.data_ptr()), S, None, None,
                                               0), tm._ctx, "pu_simulate_device")

        for i in range(args.warmup):
            call(i)
        torch.cuda.synchronize(dev)
        ms = []
        for i in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(100 + i)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        row = dict(cfg, device_ms_median=statistics.median(ms), device_ms_min=min(ms),
                   device_ms_max=max(ms), draws_per_site=2 * cfg["ntax"])
        row["device_ns_per_draw"] = 1e6 * row["device_ms_median"] / (S * row["draws_per_site"])
        if not args.no_host:
            t0 = time.perf_counter()
            synthetic.simulate_states(np.random.default_rng(1), tree, model, rm.rates, S)
            row["host_s"] = time.perf_counter() - t0
            row["speedup"] = row["host_s"] * 1e3 / row["device_ms_median"]
        result["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        N.check(N.lib().pu_ctx_set_stream(tm._ctx, N.PU_OWN_STREAM), tm._ctx)
        del tm, d_tips
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
