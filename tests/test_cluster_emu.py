"""Pose clustering on the CPU-emulated kernel library: the pose embedding against the atoms in float64, the dense RMSD kernel,
the neighbour bitmap and the greedy scan (csrc/dlpd_cluster.h) against the float64 predicate and the greedy clustering
written from the definition, planted sets, errors, ``Docker.cluster`` on a searched list and the cluster step of
scripts/dock_pair.py.  Check bodies and the derivation of the tolerances and radii: tests/cluster_checks.py."""
import pytest

import cluster_checks as cc


def test_embedding_distance_is_the_atom_rmsd():
    cc.check_embedding()


@pytest.mark.parametrize("Ka,Kb", [(1, 1), (65, 3), (200, 200)])
def test_pose_rmsd_matches_float64(emu, Ka, Kb):
    cc.check_dense(emu, "cpu", Ka, Kb)


def test_duplicated_poses_are_at_distance_zero(emu):
    cc.check_duplicates(emu, "cpu")


@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
def test_bitmap_is_the_float64_predicate(emu, K):
    cc.check_bitmap(emu, "cpu", 1, K)


@pytest.mark.parametrize("key,K", [(2, None), (4, None), (1, 130)])
def test_cluster_is_the_float64_greedy(emu, key, K):
    cc.check_cluster(emu, "cpu", key, K)


def test_cluster_edge_cases(emu):
    cc.check_cluster_edges(emu, "cpu")


def test_planted_clusters(emu):
    cc.check_planted(emu, "cpu", 130, 4)


def test_cluster_errors(emu):
    cc.check_errors(emu, "cpu")


def test_docker_cluster_on_a_searched_list(emu, tmp_path):
    cc.check_docker_cluster(emu, "cpu", 16, tmp_path)


def test_dock_pair_cluster_step(emu, tmp_path):
    cc.check_dock_pair(emu, "cpu", tmp_path)
