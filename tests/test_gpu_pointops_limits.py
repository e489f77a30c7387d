"""-m gpu: the query and sampling kernels of csrc/pointops.hip (k-NN, ball query, random ball query, farthest point sampling)
and the wrappers built on them (interpolation, query_and_group) at the places where they change behaviour: every register
bucket of the k-NN template and both sides of each bucket edge, the 2048-candidate bound of the ball query from below, on and
above it, write-out loops longer than a wave, empty scenes on either side of the scene lookup, arg-max ties across threads,
waves and the workgroup, more picks than points.

Bars: indices and distances bit-exact against oracle/pointops.py (both sides compute ((dx*dx + dy*dy) + dz*dz) in fp32 without
contraction; equal distances: lower index first).  Interpolated features and their gradient: 1e-5 * max(1, |ref|_max) against
the float64 oracle, the bar of test_pointops_edge_operators for this operator family.
"""
import numpy as np
import pytest
import torch

from oracle import pointops as opo

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)             # a copy: the shared cases are read-only


def _scene_of(offsets, row):
    return int(np.searchsorted(np.asarray(offsets), row, side="right"))


def _same(name, got, want, new_offset):
    """bit-exact rows; on a mismatch name the first differing query and its scene"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
        r = int(rows[0])
        raise AssertionError(f"{name}: {len(rows)} of {got.shape[0]} rows differ; first: query {r} (scene {_scene_of(new_offset, r)})\n"
                             f"got  {got[r]}\nwant {want[r]}")


# ---- 1. k-NN: every template bucket, both sides of every bucket edge, eight scenes ---------------------------------------------
KNN_SIZES = [1500, 0, 7, 1030, 1, 64, 300, 129]         # an empty scene; scenes smaller than nsample; 1500 and 1030: past the 1024-point tile
KNN_QUERIES = [300, 5, 40, 0, 3, 260, 1, 90]            # queries into the empty scene; a scene nobody queries; 699 = 2 * 256 + 187


@pytest.fixture(scope="module")
def knn_case():
    """the scenes and the oracle's 128 nearest of every query, computed once: the nearest nsample are its first nsample columns
    (one ascending (distance, index) order per query).  Workgroup 1 (queries 256..511) serves scenes 0, 1, 2, 4 and 5."""
    rng = np.random.default_rng(1801)
    xyz = rng.random((sum(KNN_SIZES), 3)).astype(np.float32)
    off, noff = np.cumsum(KNN_SIZES).astype(np.int32), np.cumsum(KNN_QUERIES).astype(np.int32)
    xyz[200:260] = xyz[100:160]                                       # exact ties inside scene 0 ...
    xyz[1030:1050] = xyz[1000:1020]                                   # ... across its LDS tile boundary ...
    s7 = int(off[6])
    xyz[s7 + 64:s7 + 128] = xyz[s7:s7 + 64]                           # ... and scene 7 = 64 points twice + 1: ties at ranks 2j, 2j + 1
    new_xyz = rng.random((sum(KNN_QUERIES), 3)).astype(np.float32)
    new_xyz[:20] = xyz[:20]                                           # zero distances
    new_xyz[1] = xyz[1000]
    s5, q5, q7 = int(off[4]), int(noff[4]), int(noff[6])
    new_xyz[q5:q5 + 64] = xyz[s5:s5 + 64]
    new_xyz[q7:q7 + 30] = xyz[s7:s7 + 30]
    assert len(new_xyz) % 256 != 0
    assert len({_scene_of(noff, q) for q in range(256, 512)}) >= 4
    idx, dist = opo.knn_query(128, xyz, off, new_xyz, noff)
    for a in (xyz, off, new_xyz, noff, idx, dist):
        a.setflags(write=False)
    return xyz, off, new_xyz, noff, idx, dist


@pytest.mark.parametrize("nsample", [2, 4, 5, 8, 9, 32, 33, 64, 65, 128])
def test_knn_query_register_buckets_and_their_edges(cuda, knn_case, nsample):
    """knn_query_kernel<K> for K = 4, 8, 16, 64 and 128 at nsample = K and K + 1 (the next bucket), K = 32 at both of its ends."""
    from pointcept_amd import pointops_api as po

    xyz, off, new_xyz, noff, want_i, want_d = knn_case
    got_i, got_d = po.knn_query(nsample, _t(xyz, cuda), _t(off, cuda), _t(new_xyz, cuda), _t(noff, cuda))
    want_i, want_d = np.ascontiguousarray(want_i[:, :nsample]), np.ascontiguousarray(want_d[:, :nsample])
    _same("knn idx", got_i, want_i, noff)
    _same("knn dist", got_d, want_d, noff)
    empty = slice(int(noff[0]), int(noff[1]))                          # queries into the scene without points
    assert bool((got_i[empty] == -1).all()) and bool((got_d[empty] == 1e5).all())
    small = slice(int(noff[1]), int(noff[2]))                          # 7 points
    assert bool((got_i[small, :min(nsample, 7)] >= 0).all()) and bool((got_i[small, 7:] == -1).all())


def test_knn_query_refuses_more_than_128_neighbours(cuda):
    from pointcept_amd import pointops_api as po
    from pointcept_amd._lib import PtcoreError

    x = torch.rand(200, 3, device=cuda)
    o = torch.tensor([120, 200], dtype=torch.int32, device=cuda)
    with pytest.raises(PtcoreError):
        po.knn_query(129, x, o)
    idx, dist = po.knn_query(128, x, o)
    torch.cuda.synchronize()
    assert idx.shape == (200, 128) and bool((idx[:120, :120] >= 0).all()) and bool((idx[:120, 120:] == -1).all())
    assert bool((idx[120:, :80] >= 120).all()) and bool((idx[120:, 80:] == -1).all())


# ---- 2. ball query: the 2048-candidate bound, write-out past one wave, no candidates ----------------------------------------------
BQ_SIZES = [2047, 2048, 0, 2049, 2600, 40, 16, 100, 128, 33]    # below / on / above the bound; an empty scene; 16, 100, 128: cnt == nsample
BQ_QUERIES = [5, 5, 2, 6, 7, 4, 2, 2, 2, 0]


@pytest.fixture(scope="module")
def bq_case():
    rng = np.random.default_rng(1802)
    xyz = rng.random((sum(BQ_SIZES), 3)).astype(np.float32)
    off, noff = np.cumsum(BQ_SIZES).astype(np.int32), np.cumsum(BQ_QUERIES).astype(np.int32)
    new_xyz = rng.random((sum(BQ_QUERIES), 3)).astype(np.float32)
    s, q = np.concatenate([[0], off[:-1]]), np.concatenate([[0], noff[:-1]])
    past = {}                                                          # query -> the point it copies, which lies past the bound
    new_xyz[q[0]], new_xyz[q[0] + 1] = xyz[s[0]], xyz[s[0] + 2046]     # in scenes within the bound the copied point comes first
    new_xyz[q[1]], new_xyz[q[1] + 1] = xyz[s[1]], xyz[s[1] + 2047]
    new_xyz[q[3]], new_xyz[q[3] + 1] = xyz[s[3] + 2047], xyz[s[3] + 2048]
    past[int(q[3] + 1)] = int(s[3] + 2048)
    for j, local in enumerate([2048, 2300, 2599]):
        new_xyz[q[4] + j] = xyz[s[4] + local]
        past[int(q[4] + j)] = int(s[4] + local)
    new_xyz[q[4] + 3] = xyz[s[4] + 2047]
    order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(s, off)]).astype(np.int32)
    for a in (xyz, off, new_xyz, noff, order):
        a.setflags(write=False)
    return xyz, off, new_xyz, noff, order, past


@pytest.mark.parametrize("nsample", [16, 100, 128])
def test_ball_query_at_and_over_the_candidate_bound(cuda, bq_case, nsample):
    """every point of a scene in range (unit cube, radius 10): 2047, 2048, 2049 and 2600 candidates -- the `pos < BQ_CAP` guard,
    the clamp, the early exit, the full 2048-slot sort and the padded sort of 2047; nsample > 64: the second trip of both
    write-out loops; 40 points: sub-sampled at 16, padded at 100 and 128; the scene of exactly nsample points: cnt == nsample."""
    from pointcept_amd import pointops_api as po

    xyz, off, new_xyz, noff, order, past = bq_case
    dev = [_t(a, cuda) for a in (xyz, off, new_xyz, noff)]
    want_i, want_d = opo.ball_query(nsample, 10.0, 0.0, xyz, off, new_xyz, noff)
    got_i, got_d = po.ball_query(nsample, 10.0, 0.0, *dev)
    _same("ball_query idx", got_i, want_i, noff)
    _same("ball_query dist", got_d, want_d, noff)
    got = got_i.cpu().numpy()
    for query, point in past.items():                                  # a kernel without the bound returns the copied point first
        assert point not in got[query] and got[query, 0] != point
    for query in (0, 1, int(noff[0]), int(noff[0]) + 1, int(noff[2])):
        assert float(got_d[query, 0]) == 0.0                           # within the bound the copied point is found
    exact = BQ_SIZES.index(nsample)                                    # cnt == nsample: every point once, nothing padded
    rows = got[int(noff[exact - 1]):int(noff[exact])]
    assert len(rows) == 2 and all(sorted(r) == list(range(int(off[exact - 1]), int(off[exact]))) for r in rows)
    nowhere = slice(int(noff[1]), int(noff[2]))                        # queries into the empty scene
    assert bool((got_i[nowhere] == -1).all()) and bool((got_d[nowhere] == 1e5).all())

    # the random variant stops at nsample and has no candidate bound: the first nsample points along `order`
    want_i, want_d = opo.ball_query(nsample, 10.0, 0.0, xyz, off, new_xyz, noff, order=order)
    got_i, got_d = po.random_ball_query(nsample, 10.0, 0.0, *dev, order=_t(order, cuda))
    _same("random_ball_query idx", got_i, want_i, noff)
    _same("random_ball_query dist", got_d, want_d, noff)
    s4, q4 = int(off[3]), int(noff[3])
    assert np.array_equal(got_i[q4].cpu().numpy(), order[s4:s4 + nsample])


@pytest.mark.parametrize("nsample", [16, 100])
def test_ball_query_without_candidates(cuda, nsample):
    """min_radius > 0 and queries far from every point: cnt == 0 (the two-slot sort of padding alone), every slot -1 / 1e5; two
    queries that do have candidates (and one that is a point: d2 <= 1e-5 passes whatever min_radius is) sit between them."""
    from pointcept_amd import pointops_api as po

    rng = np.random.default_rng(1803)
    sizes, queries = [300, 70], [5, 4]
    xyz = rng.random((sum(sizes), 3)).astype(np.float32)
    off, noff = np.cumsum(sizes).astype(np.int32), np.cumsum(queries).astype(np.int32)
    new_xyz = (50.0 + rng.random((sum(queries), 3))).astype(np.float32)
    new_xyz[2], new_xyz[6] = np.float32(0.5), xyz[310]
    far = [0, 1, 3, 4, 5, 7, 8]
    dev = [_t(a, cuda) for a in (xyz, off, new_xyz, noff)]
    order = _t(np.concatenate([rng.permutation(300), 300 + rng.permutation(70)]).astype(np.int32), cuda)
    for name, got, want in (("ball_query", po.ball_query(nsample, 1.0, 0.5, *dev), opo.ball_query(nsample, 1.0, 0.5, xyz, off, new_xyz, noff)),
                            ("random_ball_query", po.random_ball_query(nsample, 1.0, 0.5, *dev, order=order),
                             opo.ball_query(nsample, 1.0, 0.5, xyz, off, new_xyz, noff, order=order.cpu().numpy()))):
        _same(name + " idx", got[0], want[0], noff)
        _same(name + " dist", got[1], want[1], noff)
        assert bool((got[0][far] == -1).all()) and bool((got[1][far] == 1e5).all())
        assert int(got[0][2, 0]) >= 0 and float(got[1][2, 0]) >= 0.5
    assert int(po.ball_query(nsample, 1.0, 0.5, *dev)[0][6, 0]) == 310     # sorted: the point itself comes first


# ---- 3. farthest point sampling: ties and degenerate scenes ----------------------------------------------------------------------
def test_fps_ties_and_degenerate_scenes(cuda):
    """scene 0: 2100 points, the second half a copy of the first (every arg-max round ties between two threads -- point i and
    i + 1050 belong to threads i and i + 26 mod 1024: the same wave or the next one); scene 1: 50 identical points; scene 2: more
    picks than points; scene 3: no points, no picks; scene 4: points but no picks; scene 5: one point; scene 6: 1100 points, the
    last 76 copies of the first 76 (points k and k + 1024: a tie inside one thread's strided run).  Lower index wins everywhere."""
    from pointcept_amd import pointops_api as po

    rng = np.random.default_rng(1804)
    sizes, picks = [2100, 50, 5, 0, 30, 1, 1100], [200, 10, 9, 0, 0, 1, 30]
    xyz = rng.random((sum(sizes), 3)).astype(np.float32)
    xyz[1050:2100] = xyz[:1050]
    xyz[2100:2150] = xyz[2100].copy()
    xyz[2186 + 1024:2186 + 1100] = xyz[2186:2186 + 76]
    off, noff = np.cumsum(sizes).astype(np.int32), np.cumsum(picks).astype(np.int32)
    want = opo.farthest_point_sampling(xyz, off, noff)
    x, o, no = _t(xyz, cuda), _t(off, cuda), _t(noff, cuda)
    got = po.farthest_point_sampling(x, o, no)
    again = po.farthest_point_sampling(x, o, no)
    assert torch.equal(got, again)
    g = got.cpu().numpy()
    assert g.dtype == np.int32 and g.shape == (sum(picks),)
    if not np.array_equal(g, want):
        j = int(np.nonzero(g != want)[0][0])
        raise AssertionError(f"first difference at pick {j} (scene {_scene_of(noff, j)}): got {g[j]}, want {want[j]}")
    assert (g[:200] < 1050).all() and len(set(g[:200].tolist())) == 200      # never the copy, never a point twice
    assert (g[200:210] == 2100).all()                                         # identical points: the first index every round
    assert sorted(g[210:215].tolist()) == [2150, 2151, 2152, 2153, 2154] and (g[215:219] == 2150).all()
    assert g[219] == int(off[4])
    assert (g[220:] < 2186 + 1024).all() and len(set(g[220:].tolist())) == 30


# ---- 4. interpolation / interpolation2: forward and gradient against the float64 oracle ------------------------------------------
def _close(name, got, ref, tol=1e-5):
    """the `close` of test_pointops_edge_operators against a float64 reference"""
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, (name, got.dtype, tuple(got.shape), ref.shape)
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max())
    bar = tol * max(1.0, float(np.abs(ref).max()))
    print(f"{name}: max abs err {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("fn", ["interpolation", "interpolation2"])
@pytest.mark.parametrize("c", [5, 32])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_interpolation_forward_and_gradient(cuda, fn, k, c):
    """inverse-distance weights over the k nearest sources: three scenes, one of two points (fewer than k = 3 and 8: its -1 slots
    keep their ~1e-5 share of the normaliser and add zero), targets that are sources (distance 0: weight ~1 on that point) and
    sources that are each other's copies (equal weights)."""
    from pointcept_amd import pointops_api as po

    rng = np.random.default_rng(1805)
    sizes, targets = [150, 2, 90], [200, 30, 140]
    xyz = rng.random((sum(sizes), 3)).astype(np.float32)
    xyz[20:30] = xyz[10:20]
    new_xyz = rng.random((sum(targets), 3)).astype(np.float32)
    new_xyz[:50] = xyz[:50]
    new_xyz[200], new_xyz[230:250] = xyz[150], xyz[160:180]
    off, noff = np.cumsum(sizes).astype(np.int32), np.cumsum(targets).astype(np.int32)
    feat = rng.standard_normal((sum(sizes), c)).astype(np.float32)
    probe = rng.standard_normal((sum(targets), c)).astype(np.float32)
    want, want_grad = opo.interpolation(xyz, new_xyz, feat, off, noff, k, grad_out=probe)

    def run():
        f = _t(feat, cuda).requires_grad_(True)
        out = getattr(po, fn)(_t(xyz, cuda), _t(new_xyz, cuda), f, _t(off, cuda), _t(noff, cuda), k)
        (out * _t(probe, cuda)).sum().backward()
        return out.detach(), f.grad

    out, grad = run()
    _close(f"{fn} k={k} c={c}", out, want)
    _close(f"{fn} k={k} c={c} d_feat", grad, want_grad)
    out2, grad2 = run()
    assert torch.equal(out, out2) and torch.equal(grad, grad2), "segmented-sum gradient must be bit-reproducible"
    if k > 2:                                                           # the two-point scene: one source at distance 0 takes all the weight
        assert torch.allclose(out[200], _t(feat[150], cuda), rtol=0, atol=1e-5 * float(np.abs(feat).max()))


# ---- 5. query_and_group: which of the 1 + (nsample - 1)(dilation + 1) neighbours are kept -----------------------------------------
@pytest.mark.parametrize("nsample", [4, 8])
@pytest.mark.parametrize("dilation", [0, 2])
def test_query_and_group_dilation_columns(cuda, nsample, dilation):
    """libs/pointops/functions/utils.py:62-84: every (dilation + 1)-th neighbour, or, in a scene with fewer points than were asked
    for, the stride that still spans it (9 points: taken for dilation 2; 6 points: taken always but at nsample 4, dilation 0)."""
    from pointcept_amd import pointops_api as po

    rng = np.random.default_rng(1806)
    sizes, queries = [300, 9, 6], [70, 11, 5]
    xyz = rng.random((sum(sizes), 3)).astype(np.float32)
    new_xyz = rng.random((sum(queries), 3)).astype(np.float32)
    new_xyz[:10], new_xyz[70:73] = xyz[:10], xyz[300:303]
    off, noff = np.cumsum(sizes).astype(np.int32), np.cumsum(queries).astype(np.int32)
    total = 1 + (nsample - 1) * (dilation + 1)
    wide, _ = opo.knn_query(total, xyz, off, new_xyz, noff)
    want, q0 = [], 0
    for count, q1 in zip(sizes, noff):
        soft = (count - 1) / (nsample - 1) - 1 if count < total else dilation
        cols = [int((soft + 1) * j) for j in range(nsample)]
        assert cols[-1] <= min(count, total) - 1
        want.append(wide[q0:q1, cols])
        q0 = q1
    want = np.concatenate(want)
    x, nx, o, no = _t(xyz, cuda), _t(new_xyz, cuda), _t(off, cuda), _t(noff, cuda)
    feat = torch.randn(sum(sizes), 6, device=cuda)
    grouped, idx = po.query_and_group(nsample, x, nx, feat, None, o, no, dilation=dilation)
    _same("query_and_group idx", idx, want, noff)
    # the soft stride ends at the scene's last neighbour: no empty slot in any scene (6 points at nsample 8 repeat columns instead)
    assert bool((idx >= 0).all())
    assert grouped.shape == (sum(queries), nsample, 9) and torch.equal(grouped, po.grouping(idx, feat, x, nx, with_xyz=True))
    only_idx = po.query_and_group(nsample, x, nx, feat, None, o, no, dilation=dilation, with_feat=False)
    assert torch.equal(only_idx, idx)
    plain, _ = po.query_and_group(nsample, x, nx, feat, None, o, no, dilation=dilation, with_xyz=False)
    assert torch.equal(plain, po.grouping(idx, feat, x))
