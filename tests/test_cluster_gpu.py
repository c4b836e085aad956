"""Pose clustering on the real gfx950 build: the dense RMSD kernel, the neighbour bitmap (under guarded allocations) and the
greedy scan (csrc/dlpd_cluster.h) against float64, planted sets up to the 65,536-pose limit (a scan block of 256 threads:
K = 16,449 is the smallest list with more words than threads), errors and ``Docker.cluster`` on a searched list.  Check
bodies and the derivation of the tolerances and radii: tests/cluster_checks.py.  Nothing here reads the reference tree."""
import pytest
import torch

import cluster_checks as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from deeplocalproteindocking_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("Ka,Kb", [(1, 1), (65, 3), (200, 200), (1000, 257)])
def test_pose_rmsd_matches_float64(dev, lib, Ka, Kb):
    cc.check_dense(lib, dev, Ka, Kb)


def test_duplicated_poses_are_at_distance_zero(dev, lib):
    cc.check_duplicates(lib, dev)


@pytest.mark.parametrize("key,K", [(1, 1), (1, 63), (1, 64), (1, 65), (1, 200), (1, 300), (3, 1000)])
def test_bitmap_is_the_float64_predicate(dev, lib, key, K):
    cc.check_bitmap(lib, dev, key, K, guard=True)


@pytest.mark.parametrize("key", [1, 2, 3, 4, 5])
def test_cluster_is_the_float64_greedy(dev, lib, key):
    cc.check_cluster(lib, dev, key)


def test_cluster_edge_cases(dev, lib):
    cc.check_cluster_edges(lib, dev)


@pytest.mark.parametrize("K,ns", [(130, 4), (16449, 40), (65536, 64)])
def test_planted_clusters(dev, lib, K, ns):
    cc.check_planted(lib, dev, K, ns)


def test_cluster_errors(dev, lib):
    cc.check_errors(lib, dev)


def test_docker_cluster_on_a_searched_list(dev, tmp_path):
    cc.check_docker_cluster(None, dev, 32, tmp_path)
