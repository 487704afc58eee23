"""The GLVQ family (K9 glvq, K11 grlvq, K12 gmlvq) and batch neural gas (K10) on labelled maps that are stored in 8x8 patches.

somhip_codebook_create (csrc/somhip.hip, codebook_create) stores a map whose sides are multiples of 8 in patch order, labels
or not, and the tools hand a file's topology straight through -- so a map that vcal has labelled and glvq fine-tunes is
patch-stored.  Storage row and unit differ only from xdim 16 on (kernels/common.hpp unit_of_row: one patch per lattice
row of patches is the identity), and the replays (glvq_replay, grlvq_replay, gmlvq_replay, ngas_replay) work in unit order
and know nothing about storage: every stage is compared with them by bit pattern, as test_glvq / test_grlvq / test_gmlvq /
test_ngas do on codebooks without a lattice, and whole runs also with the same rows uploaded without a lattice.

The shapes are the smallest at which a code path differs: 16x8 (two row groups, k_scan_class<32, 1>; the smallest map that
permutes), 24x16 (three patches per row of patches: the patch row matters), 32x32 (16 row groups: the first shape on
k_scan_class<32, 4>, GLVQ_R = 4 in kernels/glvq.hpp and `wide` in host_proto.inc's class_scan_walk) and 40x40 (25 groups:
the last wave of the wide kernel holds one live group of four).  No new tolerance: the sigmoid case uses the bounds of
DESIGN.md K9 and K12 as test_glvq and test_gmlvq do.  The runs across the scan chunks are in test_lvq_family_chunks.py."""
import copy
import os
import re
import types

import numpy as np
import pytest

import glvq_replay as G
import gmlvq_replay as M
import grlvq_replay as R
import ngas_replay as N
import test_glvq as TG
import test_gmlvq as TM
import test_grlvq as TR
import test_ngas as TN
from test_glvq import built, tools                                     # noqa: F401  (fixtures)

f32, f64 = np.float32, np.float64
bits32, bits64, run = TG.bits32, TG.bits64, TG.run
HEXA, BUBBLE = TN.HEXA, TN.BUBBLE

MAPS = [(16, 8, 3), (24, 16, 5), (32, 32, 16), (40, 40, 5)]           # xdim, ydim, dim
GROUPS = {(16, 8): 2, (24, 16): 6, (32, 32): 16, (40, 40): 25}         # row groups of 64
WIDE_GROUPS = 16                                                       # 4 * GLVQ_R: from here on the search is k_scan_class<32, 4>
N_DATA = 120                                                           # no multiple of the 32-sample tile


def unit_of_row(xdim, ydim):
    """kernels/common.hpp unit_of_row over a whole patch-stored map: the unit that storage row r holds"""
    row = np.arange(xdim * ydim)
    p, i = row >> 6, row & 63
    px, py = p % (xdim // 8), p // (xdim // 8)
    return (py * 8 + (i >> 3)) * xdim + px * 8 + (i & 7)


_cases = {}


def map_case(xdim, ydim, dim):
    """test_glvq.edge_case on a map, with the edges chosen from the permutation: class 3 lies inside the last storage group,
    class 4 is the last lattice row (spread over xdim / 8 groups), class 5 has a single unit; two pairs of duplicated rows
    (u, v), u < v, with storage rows the other way round -- one within a class, one across two classes -- and samples equal
    to them in either class, so the lower unit has to win in both roles and decides `correct` where D = 0; a unit of -0.0s
    and 1000s that no sample chooses.  Built once per shape and left unchanged."""
    if (xdim, ydim, dim) in _cases:
        return _cases[(xdim, ydim, dim)]
    units = xdim * ydim
    rs = np.random.RandomState(7000 + units + dim)
    perm = unit_of_row(xdim, ydim)
    row_of = np.argsort(perm)
    c = rs.standard_normal((units, dim)).astype(f32)
    cl = rs.randint(0, 3, size=units).astype(np.int32)
    cl[perm[-32:]] = 3
    cl[units - xdim:] = 4
    plain = np.flatnonzero(cl < 3)
    single = int(plain[3])
    cl[single] = 5
    free = plain[plain != single]
    pairs = []
    for u in free:                                                     # the first two disjoint pairs whose orders disagree
        cand = free[(free > u) & (row_of[free] < row_of[u])]
        cand = [v for v in cand if not any(v in p for p in pairs)]
        if cand and not any(u in p for p in pairs):
            pairs.append((int(u), int(cand[0])))
        if len(pairs) == 2:
            break
    (u1, v1), (u2, v2) = pairs
    c[v1] = c[u1]; cl[v1] = cl[u1]
    c[v2] = c[u2]; cl[v2] = (cl[u2] + 1) % 3
    rest = [int(u) for u in free if u not in (u1, v1, u2, v2) and row_of[u] != u]
    zero = rest[-1]
    c[zero, ::2] = -0.0
    c[zero, 1::2] = 1000.0
    x = (rs.standard_normal((N_DATA, dim)) * 1.5).astype(f32)
    dl = cl[rs.randint(0, units, size=N_DATA)].astype(np.int32)
    x[0] = c[u1]; dl[0] = cl[u1]                                       # d+ = 0 on a duplicated pair
    x[1] = c[u1]; dl[1] = (cl[u1] + 1) % 3                             # d- = 0 on it
    x[2] = c[u2]; dl[2] = cl[u2]                                       # D = 0: key+ < key- by the unit alone
    x[3] = c[u2]; dl[3] = cl[v2]                                       # D = 0 the other way round
    dl[4], dl[5], dl[6] = 3, 4, 5
    x[7] = c[perm[-1]]; dl[7] = 3
    x[8] = c[units - 1]; dl[8] = 4
    x[9] = c[units - xdim]; dl[9] = 0                                  # the last lattice row's first unit, in the other role
    assert set(dl.tolist()) <= set(cl.tolist()) and set(cl.tolist()) == set(range(6))
    k = types.SimpleNamespace(xdim=xdim, ydim=ydim, dim=dim, units=units, c=c, cl=cl, x=x, dl=dl, perm=perm, row_of=row_of, pairs=pairs,
                              single=single, zero=zero)
    for a in (c, cl, x, dl, perm, row_of):
        a.setflags(write=False)
    _cases[(xdim, ydim, dim)] = k
    return k


def metrics(k):
    """(lambda, omega of a rank below dim, omega of rank dim) of a shape: a relevance vector that is not uniform and
    matrices with a weight on every column"""
    rs = np.random.RandomState(k.units * 3 + k.dim)
    lam = rs.uniform(0.05, 2.0, size=k.dim).astype(f32)
    low = max(2, k.dim // 4)
    assert low < k.dim
    return lam, (0.5 * rs.standard_normal((low, k.dim))).astype(f32), (0.5 * rs.standard_normal((k.dim, k.dim))).astype(f32)


# ------------------------------------------------------------------------------------------------ without a GPU
def test_the_wide_search_starts_where_the_shapes_say():
    """GLVQ_R and the `wide` switch of the three searches are not exposed: read from the source, so the shapes have to follow a change"""
    src = os.path.join(TG.ROOT, "som_lvq_pak_amd", "csrc")
    m = re.search(r"constexpr int GLVQ_R = (\d+);", open(os.path.join(src, "kernels", "glvq.hpp")).read())
    assert m and 4 * int(m.group(1)) == WIDE_GROUPS
    assert open(os.path.join(src, "host_proto.inc")).read().count("const bool wide = v.ngroups >= 4 * GLVQ_R;") == 1
    for name, view in (("host_glvq.inc", "cb->v"), ("host_grlvq.inc", "cb->v"), ("host_gmlvq.inc", "b.pv")):
        text = open(os.path.join(src, name)).read()                        # v: the view each search hands to the one walk
        assert "class_scan_walk(cb->e, %s, " % view in text or "class_scan_walk(e, %s, " % view in text, name
        assert not re.search(r"\bwide\b", text), name


@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_the_cases_are_patch_stored_and_permute(built, xdim, ydim, dim):
    """the guard of every test below: the shape is stored in patches (codebook_create's condition), the library's own list
    of the storage order (somhip_shard_units with two shards: the even and the odd patches) is this module's, it is not the
    identity, and the case holds the edges its docstring promises.  xdim 8 would be the identity."""
    from som_lvq_pak_amd import engine as E
    k = map_case(xdim, ydim, dim)
    units = k.units
    assert xdim % 8 == 0 and ydim % 8 == 0 and xdim >= 16
    for shard in (0, 1):
        assert np.array_equal(E.shard_units(xdim, ydim, shard, 2), k.perm.reshape(-1, 64)[shard::2].reshape(-1))
    assert np.array_equal(np.sort(k.perm), np.arange(units)) and (k.perm != np.arange(units)).sum() > units // 2
    assert np.array_equal(unit_of_row(8, 24), np.arange(192)) and np.array_equal(k.perm[k.row_of], np.arange(units))
    assert units // 64 == GROUPS[(xdim, ydim)] and (units // 64 >= WIDE_GROUPS) == (xdim >= 32)
    if (xdim, ydim) == (40, 40):
        assert (units // 64 - WIDE_GROUPS) % 4 == 1                    # the last wave of four groups holds one
    (u1, v1), (u2, v2) = k.pairs
    assert len({u1, v1, u2, v2, k.single, k.zero}) == 6
    for u, v in k.pairs:
        assert u < v and k.row_of[u] > k.row_of[v] and (bits32(k.c[u]) == bits32(k.c[v])).all()
    assert k.cl[u1] == k.cl[v1] and k.cl[u2] != k.cl[v2]
    if (xdim, ydim) == (16, 8):
        assert k.pairs[0] == (8, 16) and (k.row_of[8], k.row_of[16]) == (64, 8)
    assert (k.row_of[k.cl == 3] >= units - 64).all() and (k.cl == 3).sum() >= 16
    assert np.array_equal(np.flatnonzero(k.cl == 4), np.arange(units - xdim, units))
    assert len(set((k.row_of[k.cl == 4] >> 6).tolist())) == xdim // 8 >= 2
    assert (k.cl == 5).sum() == 1 and k.row_of[k.zero] != k.zero
    want = G.search(k.c, k.cl, k.x, k.dl)
    assert (want[1][0], want[3][1]) == (u1, u1) and (want[1][2], want[3][2]) == (u2, v2) and (want[1][3], want[3][3]) == (v2, u2)
    assert want[0][2] == 0 and want[2][2] == 0 and k.zero not in want[1] and k.zero not in want[3]
    assert set(np.flatnonzero(k.cl >= 3).tolist()) & (set(want[1].tolist()) | set(want[3].tolist()))


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    yield e
    e.close()


def on_map(E, eng, k, rows=None):
    return E.Codebook(eng, k.c if rows is None else rows, HEXA, BUBBLE, k.xdim, k.ydim, labels=k.cl)


def same_search(got, want, what):
    dp, ip, dm, im = got[:4]
    assert (ip == want[1]).all() and (im == want[3]).all(), (what, np.flatnonzero((ip != want[1]) | (im != want[3]))[:5])
    assert (bits32(dp) == bits32(want[0])).all() and (bits32(dm) == bits32(want[2])).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_search_and_projection_on_a_map(E, eng, xdim, ydim, dim):
    """glvq_search on both routes (the list route forced), grlvq_search under a lambda that is not uniform, gmlvq_search
    and gmlvq_project at a rank below dim and at rank dim; a plain and a wrapped range; winners are units, the row
    projection comes back by unit; every call twice"""
    k = map_case(xdim, ydim, dim)
    lam, om_low, om_full = metrics(k)
    cb, ds = on_map(E, eng, k), E.Dataset(eng, k.x, labels=k.dl)
    n = N_DATA
    for first in (0, N_DATA - 2):                                      # the second range wraps after two rows
        want = G.search(k.c, k.cl, k.x, k.dl, first, n)
        wantl = R.search(k.c, k.cl, k.x, k.dl, lam, first, n)
        for again in range(2):
            for route in (E.GLVQ_DIRECT, E.GLVQ_LIST):
                got = E.glvq_search(cb, ds, first, n, route)
                same_search(got, want, ("glvq", route, first))
                assert 0 <= got[4] <= n and (route == E.GLVQ_LIST or got[4] == n)
            same_search(E.grlvq_search(cb, ds, lam, first, n), wantl, ("grlvq", first))
        for om in (om_low, om_full):
            V, Y = M.project(om, k.c), M.project(om, k.x)
            wantm = G.search(V, k.cl, Y, k.dl, first, n)
            for again in range(2):
                assert (bits32(E.gmlvq_project(cb, None, om)) == bits32(V)).all(), om.shape
                assert (bits32(E.gmlvq_project(cb, ds, om, first, n)) == bits32(Y[(first + np.arange(n)) % N_DATA])).all(), (om.shape, first)
                same_search(E.gmlvq_search(cb, ds, om, first, n), wantm, ("gmlvq", om.shape, first))
    assert (bits32(cb.download()) == bits32(k.c)).all()                # unit order, and no stage wrote a row
    cb.close(); ds.close()


def same_sums(got, S, xp, xm, f, correct, keys):
    assert (bits64(got["xi_plus"]) == bits64(xp)).all() and (bits64(got["xi_minus"]) == bits64(xm)).all() and (bits64(got["f"]) == bits64(f)).all()
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    for key in keys:
        assert (bits64(got[key]) == bits64(S[key])).all(), (key, np.argwhere(bits64(got[key]) != bits64(S[key]))[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_identity_sums_on_a_map(E, eng, xdim, ydim, dim):
    """glvq_sums, grlvq_sums and gmlvq_sums over a wrapped range: xi, f, S+, S-, the counts, cost, correct, Rp, Rm and the
    relevance gradient, Gm -- all indexed by unit; every call twice"""
    k = map_case(xdim, ydim, dim)
    lam, om_low, _ = metrics(k)
    cb, ds = on_map(E, eng, k), E.Dataset(eng, k.x, labels=k.dl)
    first, n = 11, N_DATA
    dp, ip, dm, im = G.search(k.c, k.cl, k.x, k.dl, first, n)
    xp, xm, f, correct = G.terms(dp, ip, dm, im)
    assert (xp == 0).sum() >= 2                                        # the D = 0 samples are there
    S = G.sums(k.x, ip, im, xp, xm, f, k.units, first)
    Sl = TR.replay_sums(k.c, k.cl, k.x, k.dl, lam, first, n)
    Sm = TM.replay_stages(k.c, k.cl, k.x, k.dl, om_low, first, n)
    for again in range(2):
        same_sums(E.glvq_sums(cb, ds, first, n), S, xp, xm, f, correct, ("sums_plus", "sums_minus", "cost"))
        same_sums(E.grlvq_sums(cb, ds, lam, first, n), *Sl[:5], ("sums_plus", "sums_minus", "cost", "rel_plus", "rel_minus", "grad"))
        got = E.gmlvq_sums(cb, ds, om_low, first, n)
        same_sums(got, *Sm[:5], ("sums_plus", "sums_minus", "cost", "grad"))
        assert got["grad"].shape == om_low.shape and np.abs(got["grad"]).max() > 0
    special = k.cl >= 3
    assert S["n_plus"][special].sum() >= 3 and S["n_minus"][special].sum() >= 1
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_updates_on_a_map_from_the_devices_own_sums(E, eng, xdim, ydim, dim):
    """glvq_update, grlvq_update and gmlvq_update: the rows (downloaded in unit order) by bit pattern, lambda and omega after
    their steps; the unchosen unit of -0.0s keeps its bits; every call twice"""
    k = map_case(xdim, ydim, dim)
    lam, om_low, _ = metrics(k)
    cb, ds = on_map(E, eng, k), E.Dataset(eng, k.x, labels=k.dl)
    n = N_DATA
    alpha_t, eps_t = R.rate_at(7.5, 9, 2), R.rate_at(0.5, 9, 2)

    def rows_are(want, got):
        after = cb.download()
        assert (bits32(after) == bits32(want)).all(), np.argwhere(bits32(after) != bits32(want))[:5]
        assert got["n_plus"][k.zero] == 0 and got["n_minus"][k.zero] == 0
        assert (bits32(after[k.zero]) == bits32(k.c[k.zero])).all() and (bits32(after[k.zero, ::2]) == 0x80000000).all()
        unchosen = (got["n_plus"] == 0) & (got["n_minus"] == 0)
        assert (bits32(after[unchosen]) == bits32(k.c[unchosen])).all() and (bits32(after[~unchosen]) != bits32(k.c[~unchosen])).any()

    for again in range(2):
        cb.upload(k.c)
        got = E.glvq_sums(cb, ds, 0, n)
        E.glvq_update(cb, alpha_t, n, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"])
        rows_are(G.update(k.c, got, alpha_t, n), got)
        cb.upload(k.c)
        got = E.grlvq_sums(cb, ds, lam, 0, n)
        after = E.grlvq_update(cb, alpha_t, eps_t, n, lam, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"], got["grad"])
        rows_are(R.update(k.c, got, lam, alpha_t, n), got)
        assert (bits32(after) == bits32(R.relevance_step(lam, got["grad"], eps_t, n))).all() and (bits32(after) != bits32(lam)).any()
        cb.upload(k.c)
        got = E.gmlvq_sums(cb, ds, om_low, 0, n)
        after = E.gmlvq_update(cb, alpha_t, eps_t, n, om_low, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"], got["grad"])
        rows_are(M.update(k.c, got, om_low, alpha_t, n), got)
        assert (bits32(after) == bits32(M.omega_step(om_low, got["grad"], eps_t, n))).all() and (bits32(after) != bits32(om_low)).any()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_whole_runs_on_a_map_equal_the_replay_and_the_plain_codebook(E, eng, xdim, ydim, dim):
    """three epochs of glvq_train, grlvq_train and gmlvq_train over a wrapped range: rows, lambda, omega, cost and correct
    by bit pattern against the replay, from the map (twice) and from the same rows uploaded without a lattice -- storage
    order is invisible"""
    k = map_case(xdim, ydim, dim)
    _, om_low, _ = metrics(k)
    rs = np.random.RandomState(k.units)
    lam0 = rs.uniform(0.02, 0.1, size=dim).astype(f32)                 # not normalised: taken as it is
    om0 = (om_low * f32(0.5)).astype(f32)
    T, alpha, eps, first, n = 3, 5.0, 0.5, 7, N_DATA
    ds = E.Dataset(eng, k.x, labels=k.dl)
    rows, cost, correct = G.train(k.c, k.cl, k.x, k.dl, T, alpha, 0.0, first, n)
    rows_l, lam_l, cost_l, correct_l = R.train(k.c, k.cl, k.x, k.dl, lam0, T, alpha, eps, 0.0, first, n)
    rows_m, om_m, cost_m, correct_m = M.train(k.c, k.cl, k.x, k.dl, om0, T, alpha, eps, 0.0, first, n)
    assert (bits32(rows) != bits32(k.c)).any() and (bits32(lam_l) != bits32(lam0)).any() and (bits32(om_m) != bits32(om0)).any()
    for cb in (on_map(E, eng, k), on_map(E, eng, k), E.Codebook(eng, k.c, labels=k.cl)):
        gc, gr = E.glvq_train(cb, ds, T, alpha, first=first, n=n)
        assert (bits32(cb.download()) == bits32(rows)).all() and (bits64(gc) == bits64(cost)).all() and (gr == correct).all()
        cb.upload(k.c)
        gl, gc, gr = E.grlvq_train(cb, ds, T, alpha, eps, lam0, first=first, n=n)
        assert (bits32(cb.download()) == bits32(rows_l)).all() and (bits64(gc) == bits64(cost_l)).all() and (gr == correct_l).all()
        assert (bits32(gl) == bits32(lam_l)).all()
        cb.upload(k.c)
        go, gc, gr = E.gmlvq_train(cb, ds, T, alpha, eps, om0, first=first, n=n)
        assert (bits32(cb.download()) == bits32(rows_m)).all() and (bits64(gc) == bits64(cost_m)).all() and (gr == correct_m).all()
        assert (bits32(go) == bits32(om_m)).all()
        cb.close()
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", [MAPS[0], MAPS[2]])
def test_neural_gas_on_a_map(E, eng, xdim, ydim, dim):
    """K10 on 16x8 and 32x32: ng_ranks for K = 1, 5 and 12 (the duplicated pairs tie: the later unit first), ng_sums with a
    decaying weight vector over a plain and a wrapped range, three epochs of ng_train -- against ngas_replay, from the map
    and from the same rows without a lattice"""
    k = map_case(xdim, ydim, dim)
    ds = E.Dataset(eng, k.x)
    wu, wd = N.ranks(k.c, k.x, 12)
    (u1, v1), _ = k.pairs
    assert tuple(wu[0, :2]) == (v1, u1) and wd[0, 1] == 0
    want, wq = N.train(k.c, k.x, TN.schedule_of(E, k.units, 3), 3)
    for lattice in ((HEXA, BUBBLE, xdim, ydim), ()):
        cb = E.Codebook(eng, k.c, *lattice)
        for again in range(2):
            for K in (1, 5, 12):
                gu, gd = E.ng_ranks(cb, ds, K)
                assert np.array_equal(gu, wu[:, :K]), (K, np.argwhere(gu != wu[:, :K])[:8])
                TN.same(gd, wd[:, :K].copy())
        TN.same(E.ng_train(cb, ds, 3), wq)
        TN.same(cb.download(), want)
        cb.close()
        TN.check_sums(E, eng, k.c, k.x, [TN.decaying(12)], [(0, N_DATA), (N_DATA - 2, N_DATA)], lattice=lattice or None)
    ds.close()


@pytest.mark.gpu
def test_sigmoid_sums_on_a_map_within_the_derived_bounds(E, eng):
    """beta 2 on 24x16 through glvq_sums and gmlvq_sums: the bounds test_glvq and test_gmlvq take from DESIGN.md K9 and K12
    (glvq_replay.xi_rel_bound, sums_bound, gmlvq_replay.grad_bound), unchanged"""
    k = map_case(*MAPS[1])
    _, om_low, _ = metrics(k)
    cb, ds = on_map(E, eng, k), E.Dataset(eng, k.x, labels=k.dl)
    beta, n = 2.0, N_DATA
    dp, ip, dm, im = G.search(k.c, k.cl, k.x, k.dl, 0, n)
    xp, xm, f, correct = G.terms(dp, ip, dm, im, beta)
    S = G.sums(k.x, ip, im, xp, xm, f, k.units)
    Sm, xpm, xmm, fm, correctm, _ = TM.replay_stages(k.c, k.cl, k.x, k.dl, om_low, 0, n, beta)
    rel = G.xi_rel_bound(beta)
    for got, (S_, xp_, xm_, f_, correct_), grad in ((E.glvq_sums(cb, ds, 0, n, beta), (S, xp, xm, f, correct), False),
                                                    (E.gmlvq_sums(cb, ds, om_low, 0, n, beta), (Sm, xpm, xmm, fm, correctm), True)):
        worst = {}
        for name, ref, tol in (("xi_plus", xp_, rel * xp_), ("xi_minus", xm_, rel * xm_), ("f", f_, G.F_REL_BOUND * f_)):
            err = np.abs(got[name] - ref)
            worst[name] = float((err / np.maximum(tol, 1e-300)).max())
            assert (err <= tol).all(), (name, worst)
        bp, bm, bc = G.sums_bound(S_, beta)
        bounds = [("sums_plus", bp), ("sums_minus", bm), ("cost", bc)] + ([("grad", 1.001 * M.grad_bound(S_["abs_grad"], beta, n))] if grad else [])
        for name, tol in bounds:
            err = np.abs(got[name] - S_[name])
            worst[name] = float((err / tol).max())
            assert (err <= tol).all(), (name, worst)
        print("largest error / bound:", worst)
        assert (got["n_plus"] == S_["n_plus"]).all() and (got["n_minus"] == S_["n_minus"]).all() and got["correct"] == correct_
    cb.close(); ds.close()


@pytest.mark.gpu
def test_the_tools_keep_the_map_header_and_write_the_engines_rows(E, eng, tools, tmp_path):
    """glvq, grlvq and gmlvq for two epochs on a labelled 16x8 hexa map written by textio.write_entries: the output keeps
    topology, neighbourhood and sides, its labels, and holds the rows the engine leaves for the same call on the map"""
    from som_lvq_pak_amd import textio
    k = copy.copy(map_case(*MAPS[0]))
    k.c = (np.round(k.c * 16) / 16).astype(f32)                        # values that "%g" keeps; the duplicates stay duplicates
    names = ["ape", "bee", "cat", "dog", "eel", "fox"]
    dat, cod, out = tmp_path / "d.dat", tmp_path / "m.cod", tmp_path / "o.cod"
    TG.write_dat(dat, k.x, k.dl, names)
    tab = textio.LabelTable()
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = k.dim, HEXA, BUBBLE, k.xdim, k.ydim, k.c
    m.labels = [[tab.to_index(names[int(l)])] for l in k.cl]
    textio.write_entries(str(cod), m, tab)
    assert (bits32(textio.read_entries(str(cod))[0].points) == bits32(k.c)).all()
    ds = E.Dataset(eng, k.x, labels=k.dl)
    calls = (("glvq", (), lambda cb: E.glvq_train(cb, ds, 2, 2.5)),
             ("grlvq", ("-eps", 0.5), lambda cb: E.grlvq_train(cb, ds, 2, 2.5, 0.5)),
             ("gmlvq", ("-eps", 0.5), lambda cb: E.gmlvq_train(cb, ds, 2, 2.5, 0.5, E.gmlvq_omega(k.dim))))
    for tool, opt, call in calls:
        if out.exists():
            os.remove(out)
        p = run(tool, "-din", dat, "-cin", cod, "-cout", out, "-epochs", 2, "-alpha", 2.5, *opt)
        assert p.returncode == 0, (tool, p.stderr)
        cb = on_map(E, eng, k, k.c)
        call(cb)
        rows = cb.download()
        cb.close()
        assert (bits32(rows) != bits32(k.c)).any()
        head = [ln for ln in out.read_text().split("\n") if ln.strip() and not ln.startswith("#")][0]
        assert head.split() == [str(k.dim), "hexa", "16", "8", "bubble"], (tool, head)
        tab2 = textio.LabelTable()
        got = textio.read_entries(str(out), tab2)[0]
        assert (got.dim, got.topol, got.neigh, got.xdim, got.ydim) == (k.dim, HEXA, BUBBLE, 16, 8), tool
        assert [tab2.names[ls[0]] for ls in got.labels] == [names[int(l)] for l in k.cl], tool
        printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in rows], dtype=f32)     # the file is "%g" text
        assert (bits32(got.points) == bits32(printed)).all(), (tool, np.argwhere(bits32(got.points) != bits32(printed))[:5])
    ds.close()
