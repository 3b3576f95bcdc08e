"""`bench.py --gpus 2` end to end on the GPU box: no launcher environment, so bench starts
both ranks itself (bench.spawn_ranks); PU_BENCH_BACKEND=gloo puts both ranks on the one GPU
(RCCL refuses two ranks per device).  The site-sharded lnL it reports (the per-step
all-reduce, SURVEY 8(e) G1 / bin/phy.py:146's sum) must equal the one-rank lnL of the
concatenated sites, from the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_gpus2_spawns_ranks_and_sums_site_shards(oracle_mod):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PU_BENCH_BACKEND"] = "gloo"
    S = 3000
    r = subprocess.run([sys.executable, "-u", "bench.py", "--gpus", "2", "--sites", str(S),
                        "--steps", "5", "--warmup", "2", "--warm-seconds", "0", "--full",
                        "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 alone prints
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["total_sites"] == 2 * S
    assert 0 < out["roofline"]["frac"] <= 1
    # r06: the line verifies itself -- the ranks the collective spans, and the job's lnL
    # against every rank's oracle lnL summed by the same collective
    assert out["rccl_world"] == 2 and out["rank_check"]["backend"] == "gloo"
    assert out["lnl_rel_err_vs_cpu"] <= 1e-9 and out["sitewise_max_rel_err_vs_cpu"] <= 1e-9

    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, random_tree, simulate_states
    from phylo_utils_amd.tree import Traversal, prepare_tree
    model = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    rm = GammaRateModel(4, 0.5)
    tree = random_tree(np.random.default_rng(1234), 50)        # bench.py's generator
    parts = [simulate_states(np.random.default_rng(1000 + k), tree, model, rm.rates, S)
             for k in range(2)]
    tr = Traversal(prepare_tree(tree))
    eye = np.eye(4)
    tips = {node: eye[np.concatenate([p[name] for p in parts])]
            for name, node in tr.names.items()}
    ev, el, iv = model.engine_eigen()
    lnl, _ = oracle_mod.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                                 tr.root_length(), ev, el, iv, model.freqs, rm.rates, rm.weights,
                                 n_nodes=tr.n_nodes)
    assert abs(out["lnl"] - lnl) <= 1e-9 * abs(lnl), (out["lnl"], lnl)


def _bench(args, gloo=True, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    if gloo:
        env["PU_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, "-u", "bench.py"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("config,taxa,total", [("cfg2", 50, 5000), ("cfg4", 1000, 3000)])
def test_bench_strong_scaling_total_sites_fixed(config, taxa, total):
    """--total-sites: one alignment split over the ranks (strong scaling, BASELINE cfg4 as
    stated: `bench.py --gpus 8 --config cfg4 --total-sites 1000000`, rehearsed here on the
    1000-taxon cfg4 tree with 2 gloo ranks).  Two gloo ranks on the one GPU report the same
    total lnL as one rank over all sites (bin/phy.py:146's sum), `total_sites` is the same, and
    `scaling` says strong."""
    common = ["--config", config, "--total-sites", str(total), "--steps", "3", "--warmup", "1",
              "--warm-seconds", "0", "--full", "--no-cpu-baseline"]
    one = _bench(["--gpus", "1"] + common)
    two = _bench(["--gpus", "2"] + common)
    for out, n in ((one, 1), (two, 2)):
        assert out["n_gpus"] == n and out["scaling"] == "strong"
        assert out["config"]["total_sites"] == total
        assert out["config"]["updates_per_step"] == (taxa - 1) * total * 4
    assert abs(two["lnl"] - one["lnl"]) <= 1e-10 * abs(one["lnl"]), (two["lnl"], one["lnl"])
    assert two["rccl_world"] == 2 and two["lnl_rel_err_vs_cpu"] <= 1e-9
    assert abs(two["rank_check"]["lnl_job_cpu"] - one["lnl"]) <= 1e-9 * abs(one["lnl"])


def test_bench_trees_two_ranks_check_every_tree():
    """cfg5's tree-sharded line at world 2 (gloo on the one GPU, 6 trees per rank at 5000
    sites): the ranks' trees checked against the oracle, the collective's size reported; one
    rank reports a cpu_baseline and the accuracy instead."""
    common = ["--config", "cfg5", "--trees", "6", "--sites", "5000", "--steps", "3",
              "--warmup", "1", "--warm-seconds", "0", "--full", "--cpu-seconds", "5"]
    two = _bench(["--gpus", "2"] + common)
    assert two["n_gpus"] == 2 and two["config"]["total_trees"] == 12
    assert two["rccl_world"] == 2 and two["lnl_rel_err_vs_cpu"] <= 1e-9
    one = _bench(["--gpus", "1"] + common)
    assert one["cpu_baseline"]["kind"] == "port" and one["accuracy_trees"] >= 1
    assert one["lnl_rel_err_vs_cpu"] <= 1e-9


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """Without --full the line holds the headline figure and no roofline, event timing, CPU
    baseline or accuracy leg; --steps is the number of timed steps; --dump-outputs writes the
    last timed step's lnL, per-pattern lnL and root partials as float64 .npy files, identical
    from run to run (seeded inputs) and consistent with the line's lnL.  (The legs that moved
    behind --full are run by the tests above.)"""
    S = 3000
    common = ["--gpus", "1", "--sites", str(S), "--steps", "4", "--warmup", "1",
              "--warm-seconds", "0"]
    outs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        line = _bench(common + ["--dump-outputs", str(d)], gloo=False)
        assert line["steps"] == 4 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "M updates/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64"
        # value and ms_per_step describe the same timed region
        upd = line["config"]["updates_per_step"]
        assert upd == 49 * S * 4
        assert abs(line["value"] - upd / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * line["value"]
        for key in ("roofline", "timing", "cpu_baseline", "rank_check", "lnl_rel_err_vs_cpu"):
            assert key not in line, key
        arrs = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))}
        assert sorted(arrs) == ["lnl", "root_partials", "root_scale", "site_lnl"]
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64_000_000
        assert arrs["site_lnl"].shape == (S,) and arrs["root_partials"].shape == (S, 4, 4)
        assert arrs["root_scale"].shape == (S, 4)
        assert arrs["lnl"][0] == line["lnl"]
        # two fp64 sums of the same S same-signed terms: each within S * 2^-53 of the exact sum
        assert abs(arrs["site_lnl"].sum() - line["lnl"]) <= 2 * S * 2.0 ** -53 * abs(line["lnl"])
        outs.append(arrs)
    # per-site results are computed site by site, the same way in both runs: bit for bit.  The
    # lnL is their fp64 sum: at most S roundings of 2^-53 apart whatever the order
    for name in ("site_lnl", "root_partials", "root_scale"):
        np.testing.assert_array_equal(outs[0][name], outs[1][name], err_msg=name)
    assert abs(outs[0]["lnl"][0] - outs[1]["lnl"][0]) <= S * 2.0 ** -53 * abs(outs[0]["lnl"][0])
