"""The exact k-NN on a cell grid (csrc/cloud_grid.hip) and the normals and filter that run on it, against the plain
numpy fp64 references of test_gpu_cloud.py / test_gpu_densify.py: the lists must be bit-equal to brute force whatever
the cell edge and the ring limit are."""
import numpy as np
import pytest
import torch

import vslam_abi
from test_gpu_cloud import make_cloud, ref_filter, ref_knn
from test_gpu_densify import check_normals, ref_normals

pytestmark = pytest.mark.gpu


def same_lists(got, ref):
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64))
    assert np.array_equal(got[0], ref[0])


@pytest.mark.parametrize("n,k,edge,rings", [(26, 25, 0, 0), (257, 25, 0, 0), (3000, 32, 0, 0), (3000, 1, 0, 0),
                                            (3000, 25, 0.02, 2), (3000, 25, 0.02, 64), (3000, 25, 100.0, 0)])
def test_lists_bit_equal(vsctx, n, k, edge, rings):
    p = make_cloud(n, n + k)
    nbr, d2, stats = vsctx.cloud_knn_grid(p, k, edge, rings)
    print(n, k, edge, rings, "stats", stats.tolist())
    same_lists((nbr, d2), ref_knn(p, k))
    assert stats[0] + stats[1] == n
    if edge == 0.02:
        assert stats[1 if rings == 2 else 0] > 0  # an edge far too small: the pass over all points / many rings


@pytest.mark.parametrize("edge", [0, 1.0, 0.5])
def test_ties_on_cell_faces(vsctx, edge):
    g = np.arange(9.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    p = rng.permutation(np.concatenate([lat, lat[rng.choice(len(lat), 40, replace=False)]]))
    same_lists(vsctx.cloud_knn_grid(p, 25, edge)[:2], ref_knn(p, 25))


@pytest.mark.parametrize("n", [1, 2, 20])
def test_empty_slots(vsctx, n):
    p = make_cloud(20, 3)[:n]
    nbr, d2, stats = vsctx.cloud_knn_grid(p, 25)
    if n > 1:
        same_lists((nbr[:, :n - 1], d2[:, :n - 1]), ref_knn(p, n - 1))
    assert np.all(nbr[:, n - 1:] == -1) and np.all(np.isposinf(d2[:, n - 1:]))
    assert stats.sum() == n


@pytest.mark.parametrize("n,k", [(300, 20), (2500, 32)])
def test_normals_on_the_grid(vsctx, n, k):
    p = np.random.default_rng(n + k).uniform(0, 4, (n, 3))  # test_normals' clouds: the eigen-gaps are wide enough
    normals, eig = vsctx.cloud_normals(p, k, grid=True)
    check_normals(normals, eig, *ref_normals(p, k))


@pytest.mark.parametrize("box", [None, ([-0.5, -0.5, -0.5], [2.5, 1.2, 2.5])])
def test_filter_on_the_grid(vsctx, box):
    p = make_cloud(3000, 3100)
    ridx, rcounts = ref_filter(p, bbox=None if box is None else np.array(box))  # asserts the 1e-9 band empty
    out, idx, counts = vsctx.cloud_filter(p, vsctx.cloud_config(**({} if box is None else {"bbox": box})), grid=True)
    print("counts", counts.tolist(), "reference", rcounts.tolist())
    assert np.array_equal(counts, rcounts) and np.array_equal(idx, ridx)
    assert np.array_equal(out.view(np.uint64), p[ridx].view(np.uint64))


def test_beyond_the_brute_force_limit(vsctx):
    n, k = (1 << 18) + 1, 25
    p = make_cloud(n, 9)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_knn(p, k)
    nbr, d2, stats = vsctx.cloud_knn_grid(p, k)
    print("stats", stats.tolist())
    assert stats.sum() == n
    qs = np.random.default_rng(1).choice(n, 256, replace=False)
    assert np.any((p[qs] < -0.1) | (p[qs] > 2.7))  # a far outlier is among the queries
    for q in qs:
        d = p[q] - p
        r = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r[q] = np.inf
        order = np.lexsort((np.arange(n), r))[:k]
        assert np.array_equal(nbr[q], order) and np.array_equal(d2[q].view(np.uint64), r[order].view(np.uint64))


@pytest.mark.parametrize("n,k,edge,rings,code", [(600, 33, 0.0, 0, "VS_ERR_CAPACITY"),
                                                 ((1 << 23) + 1, 25, 0.0, 0, "VS_ERR_CAPACITY"),
                                                 (600, 25, -1.0, 0, "VS_ERR_ARG"), (600, 25, 0.0, -1, "VS_ERR_ARG")])
def test_errors(vsctx, n, k, edge, rings, code):
    p = make_cloud(600, 700)
    d_p = torch.from_numpy(p).cuda()
    nbr = torch.zeros((600, 33), dtype=torch.int32, device="cuda")
    d2 = torch.zeros((600, 33), dtype=torch.float64, device="cuda")
    with pytest.raises(vslam_abi.VSError, match=code):
        vsctx.cloud_knn_grid_dev(d_p.data_ptr(), n, k, nbr.data_ptr(), d2.data_ptr(), edge, rings)
    same_lists(vsctx.cloud_knn_grid(p, 25)[:2], ref_knn(p, 25))
