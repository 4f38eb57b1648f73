"""The sparse-map cloud filter on the GPU (csrc/cloud.hip; reference main.cpp:512-642, 1185-1215,
1340-1368) against plain numpy fp64: brute-force d2 = (dx dx + dy dy) + dz dz, neighbours ordered by
(d2, index) with np.lexsort, np.linalg.eigvalsh for the scatter matrix.  The k-NN lists must be
bit-equal.  The filter's keep / drop decisions must be equal wherever the tested quantity is not
within 1e-9 relative of its threshold; the reference asserts first that no point is that close
(the seeds below were picked on the CPU so that the band is empty)."""
import ctypes

import numpy as np
import pytest
import torch

import synth
import vslam_abi

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def ref_knn(p, k):
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    np.fill_diagonal(d2, np.inf)  # self excluded (main.cpp:535)
    idx = np.broadcast_to(np.arange(len(p)), d2.shape)
    order = np.lexsort((idx, d2), axis=-1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(d2, order, -1)


def _clear(value, thr):
    assert np.all(np.abs(value - thr) > 1e-9 * abs(thr)), "a point lies in the 1e-9 band: pick another seed"


def ref_sor(p, k, ratio):
    if len(p) <= k:
        return np.ones(len(p), bool)
    dist = np.sqrt(ref_knn(p, k)[1])
    md = np.zeros(len(p))
    for t in range(k):  # ascending, as main.cpp:536 sums them
        md = md + dist[:, t]
    md = md / k
    mean = md.sum() / len(p)
    thr = mean + ratio * np.sqrt(((md - mean) ** 2).sum() / len(p))
    _clear(md, thr)
    return md <= thr


def ref_surface(p, k, min_aniso):
    if len(p) <= k:
        return np.ones(len(p), bool)
    nb = p[ref_knn(p, k)[0]]  # [n, k, 3]
    c = np.zeros((len(p), 3))
    for t in range(k):
        c = c + nb[:, t]
    c = c / k
    cov = np.zeros((len(p), 3, 3))
    for t in range(k):
        d = nb[:, t] - c
        cov = cov + d[:, :, None] * d[:, None, :]
    w = np.linalg.eigvalsh(cov)
    l1, l3 = w[:, 2], w[:, 0]
    _clear(l1, 1e-12)
    aniso = 1.0 - l3 / np.maximum(l1, 1e-300)
    _clear(aniso, min_aniso)
    return (l1 >= 1e-12) & (aniso >= min_aniso)


def ref_filter(p, sor_k=25, sor_ratio=0.6, surf_k=25, surf_aniso=0.4, bbox=None, pre=None):
    idx = np.arange(len(p))
    keep = np.ones(len(p), bool) if pre is None else pre.astype(bool)
    if bbox is not None:
        keep = keep & np.all((p >= bbox[0]) & (p <= bbox[1]), axis=1)
    idx = idx[keep]
    counts = [len(idx)]
    if sor_k:
        idx = idx[ref_sor(p[idx], sor_k, sor_ratio)]
    counts.append(len(idx))
    if surf_k:
        idx = idx[ref_surface(p[idx], surf_k, surf_aniso)]
    counts.append(len(idx))
    return idx.astype(np.int32), np.array(counts, np.int32)


def make_cloud(n, seed):
    """Two planar patches with 2 mm noise, a uniform volumetric blob, 2 % far outliers; shuffled."""
    rng = np.random.default_rng(seed)
    n_out = max(1, n // 50)
    n_pl = (n - n_out) * 3 // 8
    uv = rng.uniform(0, 1.5, (2, n_pl, 2))
    a = np.column_stack([uv[0], 0.002 * rng.standard_normal(n_pl)])
    b = np.column_stack([0.002 * rng.standard_normal(n_pl) + 2.0, uv[1]])
    blob = rng.uniform(0, 0.6, (n - n_out - 2 * n_pl, 3)) + [0.5, 2.0, 1.0]
    far = rng.uniform(-6, 6, (n_out, 3))
    return rng.permutation(np.concatenate([a, b, blob, far]))


@pytest.mark.parametrize("n,k,split", [(26, 25, 0), (257, 25, 1), (1025, 25, 1), (1025, 25, 3), (3000, 32, 0),
                                       (3000, 1, 0)])
def test_knn_bit_exact(vsctx, n, k, split):
    p = np.random.default_rng(n + k).uniform(0, 4, (n, 3))
    nbr, d2 = vsctx.cloud_knn(p, k, split)
    rn, rd = ref_knn(p, k)
    assert np.array_equal(d2.view(np.uint64), rd.view(np.uint64))
    assert np.array_equal(nbr, rn)


@pytest.mark.parametrize("split", [1, 3])
def test_knn_ties_take_the_lowest_index(vsctx, split):
    g = np.arange(9.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    p = rng.permutation(np.concatenate([lat, lat[rng.choice(len(lat), 40, replace=False)]]))
    nbr, d2 = vsctx.cloud_knn(p, 25, split)
    rn, rd = ref_knn(p, 25)
    assert np.array_equal(d2.view(np.uint64), rd.view(np.uint64))
    assert np.array_equal(nbr, rn)


@pytest.mark.parametrize("split", [0, 3])
def test_knn_empty_slots(vsctx, split):
    """k above n - 1: the partial lists end in empty slots, which the merge hands on as (-1, +inf)."""
    p = np.random.default_rng(10).uniform(0, 4, (10, 3))
    nbr, d2 = vsctx.cloud_knn(p, 25, split)
    rn, rd = ref_knn(p, 9)
    assert np.array_equal(d2[:, :9].view(np.uint64), rd.view(np.uint64))
    assert np.array_equal(nbr[:, :9], rn)
    assert np.all(nbr[:, 9:] == -1) and np.all(np.isposinf(d2[:, 9:]))
    nbr, d2 = vsctx.cloud_knn(p[:1], 25, split)  # every slot empty
    assert nbr.shape == d2.shape == (1, 25)
    assert np.all(nbr == -1) and np.all(np.isposinf(d2))


CASES = {"default": {}, "box": dict(bbox=([-0.5, -0.5, -0.5], [2.5, 1.2, 2.5])), "no_sor": dict(sor_k=0),
         "no_surface": dict(surf_k=0)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [20, 26, 600, 2500])
def test_filter_equals_reference(vsctx, n, case):
    p = make_cloud(n, 100 + n)
    kw = CASES[case]
    ridx, rcounts = ref_filter(p, **{k: (np.array(v) if k == "bbox" else v) for k, v in kw.items()})
    if n == 20:
        assert rcounts[1] == rcounts[2] == rcounts[0]  # n <= k: both stages return their input
    cfg = vsctx.cloud_config(**kw)
    runs = []
    for _ in range(2):
        d_p = torch.from_numpy(p).to(DEV)
        d_out = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
        d_idx = torch.zeros(n, dtype=torch.int32, device=DEV)
        d_cnt = torch.zeros(3, dtype=torch.int32, device=DEV)
        vsctx.cloud_filter_dev(d_p.data_ptr(), n, cfg, d_out.data_ptr(), d_idx.data_ptr(), d_cnt.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        runs.append((d_out.cpu().numpy(), d_idx.cpu().numpy(), d_cnt.cpu().numpy()))
    out, idx, counts = runs[0]
    print(n, case, "counts", counts.tolist(), "reference", rcounts.tolist())
    assert np.array_equal(counts, rcounts)
    m = counts[2]
    assert np.array_equal(idx[:m], ridx)
    assert np.array_equal(out[:m].view(np.uint64), p[ridx].view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))  # run to run
    h_out, h_idx, h_counts = vsctx.cloud_filter(p, cfg)  # the host call
    assert np.array_equal(h_counts, counts) and np.array_equal(h_idx, idx[:m])
    assert np.array_equal(h_out.view(np.uint64), out[:m].view(np.uint64))
    if n >= 600 and case == "default":
        assert 0 < rcounts[2] < rcounts[1] < rcounts[0]  # both stages drop something


@pytest.fixture(scope="module")
def tracked(vsctx):
    seq = synth.sequence(24)
    feats = []
    for i in range(0, len(seq), 8):
        feats += vsctx.extract_batch([f["bgr"] for f in seq[i:i + 8]])
    S = vslam_abi.Slam(vsctx, max_batch=8)
    for i, (f, (k, d)) in enumerate(zip(seq, feats)):
        S.process_features(k, d, f["depth"], f["timestamp"], i)
    yield S
    S.close()


@pytest.mark.parametrize("valid_only", [False, True])
def test_tracker_filtered_map(tracked, valid_only):
    pos, valid = tracked.map_points()
    t = tracked.trajectory()[3]
    assert len(pos) > 50 and len(t) > 0
    ridx, rcounts = ref_filter(pos, bbox=(t.min(0) - 3.0, t.max(0) + 3.0), pre=valid if valid_only else None)
    pts, idx = tracked.filtered_map(valid_only)
    print("map", len(pos), "valid", int(valid.sum()), "reference counts", rcounts.tolist())
    assert np.array_equal(idx, ridx)
    assert np.array_equal(pts.view(np.uint64), pos[ridx].view(np.uint64))


def test_errors_are_reported_and_recoverable(vsctx):
    p = make_cloud(600, 700)
    out, idx, counts = np.zeros((600, 3)), np.zeros(600, np.int32), np.zeros(3, np.int32)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_knn(p, 33)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_filter(p, vsctx.cloud_config(surf_k=33))
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_filter(np.zeros(((1 << 18) + 1, 3)))
    rc = vsctx.lib.vs_cloud_filter(vsctx.h, p.ctypes.data_as(ctypes.c_void_p), 600, None, None,
                                   idx.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p))
    assert rc == -1  # VS_ERR_ARG
    ridx, rcounts = ref_filter(p)
    out, idx, counts = vsctx.cloud_filter(p)
    assert np.array_equal(counts, rcounts) and np.array_equal(idx, ridx)
