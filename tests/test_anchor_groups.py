"""Seed clusters and seed chains share one plan (k_clusters_plan through anchors_plan), one launch sizing and one gather of the
placed anchors above the capacity (k_anchors_large_gather).  On one CSR the two calls must therefore count the same groups,
seeds and anchors and send the same groups to the large path, whatever each does with the anchors afterwards."""
import numpy as np
import pytest

import test_seed_chains as chains
import test_seed_clusters as clusters
from test_seed_clusters import engine, big, identity_map, synthetic, u64     # noqa: F401 (engine, big: fixtures)

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 600]
SHARED = ("groups", "invalid_groups", "seeds", "anchors", "unplaced", "spilled")
COORDS = 1 << 16


@pytest.fixture(scope="module")
def csr():
    """Groups of SIZES anchors and a last one whose offsets decrease; every coordinate below 2^16, where the chains' rule
    x < 2^62 unplaces nothing that the clusters place."""
    goff, seeds, hoff, hits = synthetic(np.random.default_rng(0xA7C4), SIZES, coords=COORDS)
    assert hits.max() < COORDS and int(hoff[-1]) == sum(SIZES)
    goff = u64(list(goff) + [int(goff[-1]) - 1])
    return goff, seeds, hoff, hits


@pytest.mark.gpu
@pytest.mark.parametrize("knob, spilled", [(None, 0), ("64", 5)], ids=["default", "knob 64"])
def test_clusters_and_chains_agree_on_the_groups(big, csr, monkeypatch, knob, spilled):
    goff, seeds, hoff, hits = csr
    cmap = identity_map(COORDS)
    P = chains.params()
    n = goff.shape[0] - 1
    if knob is not None:
        monkeypatch.setenv("GCSA2_CLUSTER_LDS", knob)
        monkeypatch.setenv("GCSA2_CHAIN_LDS", knob)
    a = clusters.DeviceCsr(goff, seeds, hoff, hits)
    out_a = clusters.Outputs(n, 5)
    stats_a = a.call(big, 0, cmap, 7, 5, out_a)
    b = chains.DeviceCsr(goff, seeds, hoff, hits)
    out_b = chains.Outputs(n, P)
    stats_b = b.call(big, 0, cmap, P, out_b)
    assert {f: stats_a[f] for f in SHARED} == {f: stats_b[f] for f in SHARED}, (stats_a, stats_b)
    assert stats_a["spilled"] == spilled == sum(s > 64 for s in SIZES) * (knob is not None)
    # what the CSR alone says: one invalid group, the seeds of the others, every anchor placed by the identity map
    assert (stats_a["groups"], stats_a["invalid_groups"], stats_a["seeds"]) == (n, 1, int(goff[n - 1]))
    assert (stats_a["anchors"], stats_a["unplaced"]) == (sum(SIZES), 0)
    sums_a = out_a.arrays()[1]
    sums_b = out_b.arrays()["sums"][:n * 3].reshape(n, 3)
    assert (sums_a[:, :2] == sums_b[:, :2]).all(), (sums_a.tolist(), sums_b.tolist())
    assert sums_a[:, 0].tolist() == SIZES + [0] and not sums_a[:, 1].any()
