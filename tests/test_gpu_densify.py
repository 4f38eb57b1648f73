"""Surface densification and normals on the GPU (csrc/densify.hip; reference main.cpp:645-672,
846-965) against a plain numpy fp64 restatement: np.linalg.eigh, the same sign rule (largest component
positive), python loops for the lattice, a dict for the voxel map.  The device's Jacobi and LAPACK differ in the
last bits of the eigenvectors, so the restatement asserts on its input that every eigen-gap a used vector depends
on is >= 1e-5 l1 (axes then agree to ~1e-10, candidates to ~1e-11 m) and that no tested quantity lies within 1e-8
(relative) of its threshold; the seeds were picked on the CPU so that these hold."""
import ctypes

import numpy as np
import pytest
import torch

import vslam_abi

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = "pick another seed"
MAX_NB = 512  # VS_DENSIFY_MAX_NEIGHBOURS


def _clear(value, thr, tol=1e-8):
    assert np.all(np.abs(np.asarray(value) - thr) > tol * abs(thr)), "a value lies in the 1e-8 band: " + SEED


def orient(v):
    lead = np.take_along_axis(v, np.argmax(np.abs(v), -1)[..., None], -1)  # argmax: the lowest index on ties
    return v * np.where(lead < 0, -1.0, 1.0)


def dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def ref_normals(p, k):
    n, found = len(p), min(k, len(p))
    if found < 3:
        return np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros((n, 3))
    d2 = dist2(p[:, None, :], p[None, :, :])
    np.fill_diagonal(d2, -1.0)  # the point itself first
    order = np.lexsort((np.broadcast_to(np.arange(n), d2.shape), d2), axis=-1)[:, :found]
    nb = p[order]
    c = np.zeros((n, 3))
    for t in range(found):
        c = c + nb[:, t]
    c = c / found
    cov = np.zeros((n, 3, 3))
    for t in range(found):
        d = nb[:, t] - c
        cov = cov + d[:, :, None] * d[:, None, :]
    w, V = np.linalg.eigh(cov)
    assert np.all(w[:, 1] - w[:, 0] >= 1e-5 * w[:, 2]), "a normal's eigen-gap is too small: " + SEED
    return orient(V[:, :, 0]), w[:, ::-1]


def lattice(proj, step):
    """for (u = min; u <= max; u += step): the values, built by repeated addition."""
    vals, u = [], proj.min()
    while u <= proj.max():
        vals.append(u)
        u += step
    _clear(np.array(vals + [u]), proj.max())
    return np.array(vals)


def ref_densify(p, r=0.12, step=0.05, thresh=0.95):
    """-> (points, src, counts [4]) in insertion order."""
    n = len(p)
    if n < 20:
        return p.copy(), np.arange(n, dtype=np.int32), np.array([n, 0, n, 0], np.int32)
    N = ref_normals(p, 20)[0]
    r2 = r * r
    D2 = dist2(p[:, None, :], p[None, :, :])
    _clear(D2, r2)
    pts, src, skipped = [p], [np.arange(n)], 0
    for i in range(n):
        match = np.nonzero(D2[i] < r2)[0]
        if len(match) > MAX_NB:  # the device's cap (the reference has none)
            skipped += 1
            continue
        order = match[np.lexsort((match, D2[i, match]))]
        order = order[order != i]
        dots = np.abs((N[i, 0] * N[order, 0] + N[i, 1] * N[order, 1]) + N[i, 2] * N[order, 2])
        _clear(dots, thresh)
        co = np.concatenate([p[i:i + 1], p[order[dots >= thresh]]])
        if len(co) < 4:
            continue
        c = co.sum(0) / len(co)
        d = co - c
        w, V = np.linalg.eigh(d.T @ d)
        l1, l2, l3 = w[2], w[1], w[0]
        _clear(l1, 1e-12)
        if l1 < 1e-12:
            continue
        _clear(l3 / l1, 0.15)
        if l3 / l1 > 0.15:
            continue
        assert l1 - l2 >= 1e-5 * l1 and l2 - l3 >= 1e-5 * l1, "an axis' eigen-gap is too small: " + SEED
        ua, va = orient(V[:, 2]), orient(V[:, 1])
        pu, pv = (d[:, 0] * ua[0] + d[:, 1] * ua[1]) + d[:, 2] * ua[2], (d[:, 0] * va[0] + d[:, 1] * va[1]) + d[:, 2] * va[2]
        local = p[D2[i] < 4.0 * r2]  # every input point that can be near a candidate which passes the near test
        us, vs = lattice(pu, step), lattice(pv, step)
        cand = (c + us[:, None, None] * ua) + vs[None, :, None] * va  # [iu][iv][3]
        dco = dist2(cand[:, :, None, :], co)
        _clear(dco, r2 * 0.5)
        near = np.any(dco < r2 * 0.5, axis=-1)
        dmin = dist2(cand[near][:, None, :], local).min(-1)  # a candidate that is not near is dropped anyway
        _clear(dmin, step * step * 0.2)
        good = cand[near][~(dmin < step * step * 0.2)]  # row-major: by (u step, v step)
        pts.append(good)
        src.append(np.full(len(good), -(i + 1)))
    pts, src = np.concatenate(pts), np.concatenate(src).astype(np.int32)
    q = pts / (step * 0.7)
    assert np.all(np.abs(q - np.round(q)) > 1e-8), "a coordinate lies on a voxel face: " + SEED
    seen, keep = set(), []
    for e, key in enumerate(map(tuple, np.floor(q).astype(np.int64))):
        if key not in seen:
            seen.add(key)
            keep.append(e)
    keep = np.array(keep)
    kept_in = int((keep < n).sum())
    return pts[keep], src[keep], np.array([kept_in, len(keep) - kept_in, len(keep), skipped], np.int32)


def plane_uv(rng, m, side):
    """m points on a side x side square with a hole (radius 0.1) and a strip that keeps one point in five."""
    uv = rng.uniform(0, side, (8 * m, 2))
    hole = np.hypot(uv[:, 0] - 0.5 * side, uv[:, 1] - 0.5 * side) < min(0.1, 0.2 * side)
    strip = (uv[:, 0] > 0.75 * side) & (uv[:, 0] < 0.9 * side) & (rng.uniform(size=len(uv)) > 0.2)
    return uv[~hole & ~strip][:m]


def make_cloud(n, seed):
    """Two planar patches (2 mm noise, ~400 points / m^2), a volumetric blob, 2 % far outliers; shuffled."""
    rng = np.random.default_rng(seed)
    n_out = max(1, n // 50)
    n_pl = (n - n_out) * 3 // 8
    side = np.sqrt(n_pl / 400.0)
    uv = [plane_uv(rng, n_pl, side) for _ in range(2)]
    a = np.column_stack([uv[0], 0.002 * rng.standard_normal(n_pl)])
    b = np.column_stack([0.002 * rng.standard_normal(n_pl) + side + 0.5, uv[1]])
    n_b = n - n_out - 2 * n_pl
    blob = rng.uniform(0, (n_b / 2800.0) ** (1 / 3), (n_b, 3)) + [0.5, side + 0.5, 1.0]
    far = rng.uniform(-6, 6, (n_out, 3))
    return rng.permutation(np.concatenate([a, b, blob, far]))


def check_normals(normals, eig, rn, re):
    assert np.all(np.abs(eig - re) <= 1e-12 * re[:, :1])
    assert np.all(np.abs(normals - rn) <= 1e-9)
    assert np.all(np.take_along_axis(normals, np.argmax(np.abs(normals), -1)[:, None], -1) > 0)


@pytest.mark.parametrize("n,k", [(2, 20), (3, 20), (19, 20), (300, 20), (2500, 32)])
def test_normals(vsctx, n, k):
    p = np.random.default_rng(n + k).uniform(0, 4, (n, 3))
    rn, re = ref_normals(p, k)
    normals, eig = vsctx.cloud_normals(p, k)
    if n < 3:
        assert np.array_equal(normals, np.tile([0.0, 0.0, 1.0], (n, 1))) and not eig.any()
    check_normals(normals, eig, rn, re)


def device_run(vsctx, p, cfg, cap):
    n = len(p)
    d_p = torch.from_numpy(p).to(DEV)
    d_out = torch.zeros((cap, 3), dtype=torch.float64, device=DEV)
    d_src = torch.zeros(cap, dtype=torch.int32, device=DEV)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    vsctx.cloud_densify_dev(d_p.data_ptr(), n, cfg, cap, d_out.data_ptr(), d_src.data_ptr(), d_cnt.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_src.cpu().numpy(), d_cnt.cpu().numpy()


def check_densified(p, out, src, counts, ref):
    rout, rsrc, rcounts = ref
    print(len(p), "counts", counts.tolist(), "reference", rcounts.tolist())
    assert np.array_equal(counts, rcounts)
    assert np.array_equal(src, rsrc)
    own = src >= 0
    assert np.array_equal(out[own].view(np.uint64), p[src[own]].view(np.uint64))
    assert np.all(np.abs(out - rout) <= 1e-9)


@pytest.mark.parametrize("n,step,seed", [(19, 0.05, 319), (20, 0.05, 320), (400, 0.05, 700), (2500, 0.05, 2800),
                                         (400, 0.03, 701)])
def test_densify_equals_reference(vsctx, n, step, seed):
    p = make_cloud(n, seed)
    ref = ref_densify(p, step=step)
    cfg = vsctx.densify_config(fill_step=step)
    cap = n * 82
    runs = [device_run(vsctx, p, cfg, cap) for _ in range(2)]
    out, src, counts = runs[0]
    m = counts[2]
    check_densified(p, out[:m], src[:m], counts, ref)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(runs[0], runs[1]))  # run to run
    h_out, h_src, h_counts = vsctx.cloud_densify(p, cfg)  # the host call
    assert np.array_equal(h_counts, counts) and np.array_equal(h_src, src[:m])
    assert np.array_equal(h_out.view(np.uint64), out[:m].view(np.uint64))
    if n == 19:
        assert np.array_equal(out[:m].view(np.uint64), p.view(np.uint64)) and np.array_equal(src[:m], np.arange(n))
    if n >= 400:
        assert counts[1] > 0 and counts[0] < n  # something is filled, something is de-duplicated


def test_neighbour_cap(vsctx):
    rng = np.random.default_rng(11)
    p = make_cloud(400, 311)
    cluster = rng.uniform(0, 0.06, (560, 3)) + [0.3, 0.3, 0.0]  # on the first plane, all inside one radius
    p = rng.permutation(np.concatenate([p, cluster]))
    ref = ref_densify(p)
    assert ref[2][3] >= 560
    out, src, counts = vsctx.cloud_densify(p)
    check_densified(p, out, src, counts, ref)


def test_errors_are_reported_and_recoverable(vsctx):
    p = make_cloud(400, 700)
    ref = ref_densify(p)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_normals(p, 33)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_normals(np.zeros(((1 << 18) + 1, 3)), 20)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):
        vsctx.cloud_densify(np.zeros(((1 << 18) + 1, 3)), cap=8)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_CAPACITY"):  # 25 x 25 lattice nodes > VS_DENSIFY_MAX_GRID
        vsctx.cloud_densify(p, vsctx.densify_config(fill_step=0.01), cap=8)
    src, counts = np.zeros(400, np.int32), np.zeros(4, np.int32)
    rc = vsctx.lib.vs_cloud_densify(vsctx.h, p.ctypes.data_as(ctypes.c_void_p), 400, None, 400, None,
                                    src.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p))
    assert rc == -1  # VS_ERR_ARG
    cap = ref[2][2] // 2  # smaller than the total: the prefix is written, the total reported
    out, src, counts = vsctx.cloud_densify(p, cap=cap)
    assert np.array_equal(counts, ref[2]) and len(out) == cap
    assert np.array_equal(src, ref[1][:cap]) and np.all(np.abs(out - ref[0][:cap]) <= 1e-9)
    out, src, counts = vsctx.cloud_densify(p)
    check_densified(p, out, src, counts, ref)
