"""The fan triangulation on the GPU (csrc/cloud_mesh.hip; reference main.cpp:689-774 compute_mesh) against a plain
numpy fp64 restatement: np.lexsort for (d2, index) and (angle, list position), np.arctan2.  The device's atan2 and
glibc's differ in the last bits, so the restatement asserts on its input that no tested quantity lies within 1e-9
(relative) of its threshold and that no two angles of one fan are within 1e-9 rad; the seeds were checked on the CPU.
The index list must then equal the reference's exactly, order included."""
import functools

import numpy as np
import pytest
import torch

import vslam_abi
from test_gpu_densify import dist2, make_cloud, ref_normals

pytestmark = pytest.mark.gpu

BAND = "a value lies in the 1e-9 band: pick another seed"


def clear(value, thr):
    assert np.all(np.abs(np.asarray(value) - thr) > 1e-9 * abs(thr)), BAND


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def ref_mesh(p, N, k=20, max_edge=0.12, thresh=0.5, max_gap=1.2):
    """-> (tri [T, 3] int32 by centre point, then fan position; counts [2])."""
    n, me2, tri, fans = len(p), max_edge * max_edge, [], 0
    if n >= 3:
        D2 = dist2(p[:, None, :], p[None, :, :])
        np.fill_diagonal(D2, np.inf)
    for i in range(n if n >= 3 else 0):
        nb = np.lexsort((np.arange(n), D2[i]))[:min(k, n) - 1]
        ni, a = N[i], np.abs(N[i])
        up = np.eye(3)[0 if a[0] <= a[1] and a[0] <= a[2] else 1 if a[1] <= a[2] else 2]
        u = cross(ni, up)
        u = u / np.sqrt(dot3(u, u)) if dot3(u, u) > 0 else u
        v = cross(ni, u)
        dots = np.abs(dot3(ni, N[nb]))
        clear(D2[i, nb], me2)
        clear(dots, thresh)
        ok = nb[~(D2[i, nb] > me2) & ~(dots < thresh)]
        if len(ok) < 2:
            continue
        d = p[ok] - p[i]
        ang = np.arctan2(dot3(d, v), dot3(d, u))
        order = np.lexsort((np.arange(len(ok)), ang))
        ok, ang = ok[order], ang[order]
        assert np.all(np.diff(ang) > 1e-9), BAND
        nxt = np.roll(np.arange(len(ok)), -1)
        gap = ang[nxt] - ang
        gap[-1] += 2.0 * np.pi
        e2 = dist2(p[ok], p[ok[nxt]])
        clear(gap, max_gap)
        clear(e2, me2 * 2.5)
        emit = ~(gap > max_gap) & ~(e2 > me2 * 2.5)
        tri.append(np.column_stack([np.full(emit.sum(), i), ok[emit], ok[nxt][emit]]))
        fans += bool(emit.any())
    tri = np.concatenate(tri) if tri else np.zeros((0, 3))
    return tri.astype(np.int32), np.array([len(tri), fans], np.int32)


@functools.lru_cache(maxsize=None)
def case(n, seed, k=20, field="cloud"):
    """(points, normals, reference triangles, reference counts), computed once per case."""
    p = make_cloud(n, seed) if n >= 300 else np.random.default_rng(seed).uniform(0, 0.15, (n, 3))
    rng = np.random.default_rng(seed + 100)
    if field == "cloud":
        N = ref_normals(p, 20)[0]
    elif field == "z":
        N = np.tile([0.0, 0.0, 1.0], (n, 1))
    else:
        N = rng.standard_normal((n, 3))
        N /= np.linalg.norm(N, axis=1, keepdims=True)
    if field != "cloud":
        N[n // 3] = 0.0  # a zero normal: no fan of its own, no neighbour of anyone's
    return (p, N) + ref_mesh(p, N, k)


def device_run(vsctx, p, N, cfg, cap, n=None):
    """vs_cloud_mesh_dev on torch buffers -> (tri [cap + 16, 3] pre-filled with -7, counts)."""
    d_p, d_n = torch.from_numpy(p).cuda(), torch.from_numpy(N).cuda()
    tri = torch.full((cap + 16, 3), -7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    vsctx.cloud_mesh_dev(d_p.data_ptr(), d_n.data_ptr(), len(p) if n is None else n, cfg, cap, tri.data_ptr(),
                         cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tri.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("n,seed,k", [(19, 2, 20), (300, 3, 20), (3000, 4, 20), (3000, 5, 32), (3000, 7, 3), (2, 1, 20),
                                      (3, 1, 20)])
def test_mesh_equals_reference(vsctx, n, seed, k, grid):
    p, N, rtri, rcounts = case(n, seed, k)
    tri, counts = vsctx.cloud_mesh(p, N, grid=grid, k=k)
    print(n, k, grid, "counts", counts.tolist(), "reference", rcounts.tolist())
    assert np.array_equal(counts, rcounts) and np.array_equal(tri, rtri)
    assert (len(rtri) > 0) == (n > 3)
    if (n, k) == (3000, 20):  # a full fan and an empty one exist, so some wave holds both kinds
        per_point = np.bincount(rtri[:, 0], minlength=n)
        assert per_point.max() == k - 1 and per_point.min() == 0


@pytest.mark.parametrize("field", ["z", "random"])
def test_given_normals(vsctx, field):
    p, N, rtri, rcounts = case(300, 3, field=field)
    assert not np.array_equal(rtri, case(300, 3)[2])  # the caller's normals decide, not the cloud's
    tri, counts = vsctx.cloud_mesh(p, N)
    assert np.array_equal(counts, rcounts) and np.array_equal(tri, rtri)
    assert len(tri) > 0 and not np.any(tri == 100)  # the zero normal's point: in no triangle


def test_cap_and_order(vsctx):
    p, N, rtri, rcounts = case(300, 3)
    T, cap = len(rtri), len(rtri) // 2
    tri, counts = device_run(vsctx, p, N, None, cap)
    assert np.array_equal(counts, rcounts) and counts[0] == T
    assert np.array_equal(tri[:cap], rtri[:cap]) and np.all(tri[cap:] == -7)  # the rest of the buffer is untouched
    h_tri, h_counts = vsctx.cloud_mesh(p, N, cap=cap)  # the host call
    assert np.array_equal(h_counts, rcounts) and np.array_equal(h_tri, rtri[:cap])


def test_default_chain(vsctx):
    p = case(300, 3)[0]
    normals = vsctx.cloud_normals(p, 20)[0]
    tri, counts, used, verts, vnrm = vsctx.cloud_mesh(p, gather=True)
    rtri, rcounts = vsctx.cloud_mesh(p, normals)
    assert np.array_equal(used.view(np.uint64), normals.view(np.uint64))
    assert np.array_equal(counts, rcounts) and np.array_equal(tri, rtri) and len(tri) > 0
    assert np.array_equal(verts, p[tri]) and np.array_equal(vnrm, normals[tri])


def test_errors(vsctx):
    p, N, rtri, rcounts = case(300, 3)
    for bad, code in [({"k": 1}, "VS_ERR_ARG"), ({"max_edge": 0.0}, "VS_ERR_ARG"), ({"k": 33}, "VS_ERR_CAPACITY")]:
        with pytest.raises(vslam_abi.VSError, match=code):
            device_run(vsctx, p, N, vsctx.mesh_config(**bad), 8)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        device_run(vsctx, p, N, None, 8, n=(1 << 18) + 1)  # the n argument alone inflated: refused before any read
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_ARG"):
        vsctx.cloud_mesh_dev(torch.from_numpy(p).cuda().data_ptr(), None, 300, None, 0, None,
                             torch.zeros(2, dtype=torch.int32, device="cuda").data_ptr())
    tri, counts = vsctx.cloud_mesh(p, N)
    assert np.array_equal(counts, rcounts) and np.array_equal(tri, rtri)
