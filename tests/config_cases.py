"""The scoring configurations shared by test_score_ref.py (CPU: the oracle against score_ref.py, the residue conditions)
and test_config_space.py (GPU: the engine against the oracle)."""
import weighted_boundary as wb
from koordinator_amd import abi
from koordinator_amd.config import (BATCH_CPU, BATCH_MEMORY, CPU, GPU_MEMORY, GPU_MEMORY_RATIO, MEMORY,  # noqa: F401
                                    LoadAwareArgs, bench_profile)
from koordinator_amd.config import config5_profile as config5  # noqa: F401

# (20, 21, 41, 40): the pod kinds' weight sums are 41, 81, 82 and 122. For W = 41, 82 and 122 the float32 nearest to
# 0.5 / W lies below it by enough that 2 q W x that float rounds to just under q for many q <= 100: at residue 0 only
# the "+ 1" of the 2 S + 1 numerator keeps the truncation at q (for the other vectors' sums it would be right without)
NRF_VECTORS = [(1, 1, 1, 1), (4096, 4096, 4096, 4096), (4095, 4096, 4093, 4091), (1, 4096, 0, 3), (3, 5, 7, 11),
               (20, 21, 41, 40)]
LA_VECTORS = [(1, 1, 0), (4096, 0, 0), (1365, 1365, 1366), (0, 0, 7), (2047, 2048, 1), (0, 0, 0)]
NUMA_VECTORS = [(1, 1), (4096, 4095), (0, 5), (4096, 4096)]
PLUGIN_WEIGHTS = [(1, 1, 1), (3, 0, 7), (5000, 1, 100), (1 << 20, 1 << 20, 1 << 20)]


def with_nrf(cfg, ws):
    cfg.nrf_resources = [(n, w) for n, w in zip((CPU, MEMORY, BATCH_CPU, BATCH_MEMORY), ws) if w]
    return cfg


def with_la(cfg, ws, prod=False):
    cfg.loadaware = LoadAwareArgs(resource_weights={n: w for n, w in zip((CPU, MEMORY), ws[:2]) if w},
                                  dominant_resource_weight=ws[2], score_according_prod_usage=prod)
    if not any(ws):  # "all zero disables the score": an explicit empty weight map with a zero dominant weight
        cfg.loadaware.resource_weights = {CPU: 0, MEMORY: 0}
    return cfg


def with_numa(cfg, ws):
    cfg.numa_scoring = [(CPU, ws[0]), (MEMORY, ws[1])]
    cfg.numa_hint_scoring = [(CPU, ws[0]), (MEMORY, ws[1])]
    return cfg


def with_plugin_weights(cfg, ws):
    cfg.weight_nrf, cfg.weight_la, cfg.weight_numa = ws
    return cfg


def weight_cases():
    """(id, SchedulerConfig, the means the case claims to exercise) of §3b."""
    out = []
    for ws in NRF_VECTORS:
        out.append(("nrf-" + wb.residue_id("nrf", ws), with_nrf(bench_profile(), ws), ("nrf",)))
    for ws in LA_VECTORS:
        out.append(("la-" + wb.residue_id("la", ws), with_la(bench_profile(), ws), ("la",) if any(ws) else ()))
    out.append(("la-prod-" + wb.residue_id("la", (2047, 2048, 1)), with_la(bench_profile(), (2047, 2048, 1), prod=True), ("la",)))
    for ws in NUMA_VECTORS:
        out.append(("numa-" + wb.residue_id("numa", ws), with_numa(bench_profile(), ws), ("numa", "zone")))
    for ws in PLUGIN_WEIGHTS:
        cfg = with_numa(with_la(with_nrf(bench_profile(), (3, 5, 7, 11)), (2047, 2048, 1)), (4096, 4095))
        out.append(("plugins-" + "_".join(map(str, ws)), with_plugin_weights(cfg, ws), ("nrf", "la", "numa", "zone")))
    return out


def heavy():
    """The heavy-weight configuration the replay and whole-cluster cases reuse."""
    cfg = with_numa(with_la(with_nrf(bench_profile(), (4095, 4096, 4093, 4091)), (1365, 1365, 1366)), (4096, 4095))
    return with_plugin_weights(cfg, (5000, 1, 100))


def switch_cases():
    """(id, SchedulerConfig) of §3c: every one is past the fast path's weight domain (weights_small false)."""
    out = [("nrf_w_4097", with_nrf(bench_profile(), (4097, 1, 1, 1))),
           ("la_sum_4097", with_la(bench_profile(), (2048, 2048, 1))),
           ("numa_w_2p20", with_numa(bench_profile(), (1 << 20, 3)))]
    c = bench_profile()
    c.nrf_most = (CPU,)
    out.append(("nrf_most_cpu", c))
    c = bench_profile()
    c.numa_strategy = c.numa_hint_strategy = "MostAllocated"
    out.append(("numa_most", c))
    c = bench_profile()
    c.nrf_ignored = (BATCH_MEMORY,)
    out.append(("nrf_ignored_sc1", c))
    return out


def only(cfg, plugin):
    """cfg's KgConfig with one base plugin enabled."""
    kc = cfg.kg_config()
    kc.plugins = plugin
    return kc


PLUGIN_OF = {"nrf": abi.KG_PLUGIN_NRF, "la": abi.KG_PLUGIN_LA, "numa": abi.KG_PLUGIN_NUMA, "zone": abi.KG_PLUGIN_NUMA}
