"""Batch Robust Soft LVQ (K13) on labelled maps that are stored in 8x8 patches.

glvq_check lets a patch-stored codebook through to somhip_rslvq_train, and K13 meets storage order in two places:
k_rslvq_posterior reads dist[row_of_unit(cb, j)] (k_knn_dist writes by storage row) but labels, keys and the columns of Q
by unit j, and k_rslvq_update reads [G | c] at unit_of_row(cb, row).  Every codebook of test_rslvq.py has no lattice, where
both are the identity.  The cases, the shapes and the guard are test_lvq_family_layouts.py's: 16x8, 24x16, 32x32 and 40x40
are 2, 6, 16 and 25 row groups, so k_knn_dist runs with up to seven grid.y blocks, k_rslvq_sums with up to 25 workgroups
along grid.x and the posterior's three streams over up to 25 strides, which no test of test_rslvq.py's first shapes
reaches.  The replay (rslvq_replay) works in unit order and knows nothing about storage; its bounds are taken as they are,
and what the definition promises bit for bit -- the chunk, the storage order, an epoch and its stages -- is compared by
bit pattern.  sigma2 = dim keeps every P(y | x) of the cases above 8e-4 (test_the_replay_keeps_every_posterior_alive)."""
import copy

import numpy as np
import pytest

import rslvq_replay as R
import test_lvq_family_layouts as L
import test_rslvq as TR
from test_lvq_family_layouts import test_the_cases_are_patch_stored_and_permute    # noqa: F401  (the guard of every test below)
from test_rslvq import built, tools                                                 # noqa: F401  (fixtures)

f32, f64 = np.float32, np.float64
bits32, bits64, run = TR.bits32, TR.bits64, TR.run
MAPS, N_DATA, map_case, on_map = L.MAPS, L.N_DATA, L.map_case, L.on_map
T, ALPHA, FIRST = 3, 5.0, 7                                            # the whole runs: three epochs over a wrapped range


def run_sample(row, first):
    """the run sample that is data row `row` of a run of N_DATA samples from `first`"""
    return (row - first) % N_DATA


# ------------------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_the_replay_keeps_every_posterior_alive(xdim, ydim, dim):
    """at sigma2 = dim no P(y | x) of a case comes near underflow, samples 2 and 3 lie at distance 0 from both rows of the
    pair across two classes -- the lower unit decides `correct`, and its storage row is the higher one -- and the pair
    within a class receives the same coefficients from every sample"""
    k = map_case(xdim, ydim, dim)
    (u1, v1), (u2, v2) = k.pairs
    p = R.posterior(k.c, k.cl, k.x, k.dl, float(dim))
    assert p["pown"].min() > 8e-4
    for s in (2, 3):
        assert p["d"][s, u2] == 0 and p["d"][s, v2] == 0 and (p["d"][s] == 0).sum() == 2
    assert p["correct"][2] == 1 and p["correct"][3] == 0 and u2 < v2 and k.row_of[u2] > k.row_of[v2]
    assert (bits64(p["q"][:, u1]) == bits64(p["q"][:, v1])).all() and p["own"][0, u1] and not p["own"][1, u1]


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


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_posterior_on_a_map(E, eng, xdim, ydim, dim):
    """test_rslvq.check_posterior on the map, over a plain and a wrapped range: correct exactly, q, cost and pown within
    posterior_bounds, the invariants, chunk 64 and the rule's chunk and a second call by bit pattern.  Where D = 0 across
    two classes the lower unit wins; the pair within a class has one column of q twice; no stage writes a row."""
    k = map_case(xdim, ydim, dim)
    (u1, v1), (u2, v2) = k.pairs
    cb = on_map(E, eng, k)
    for first in (0, N_DATA - 2):                                      # the second range wraps after two rows
        got, p = TR.check_posterior(E, eng, k.c, k.cl, k.x, k.dl, float(dim), first, N_DATA, (xdim, ydim, dim, first), cb)
        s = [run_sample(row, first) for row in range(4)]
        assert got["correct"][s[2]] == 1 and got["correct"][s[3]] == 0
        q = got["q"]
        assert bits64(q[s[0], v1]) == bits64(q[s[0], u1]) and bits64(q[s[1], v1]) == bits64(q[s[1], u1])
        assert (bits64(q[:, v1]) == bits64(q[:, u1])).all() and q[s[0], u1] > 0 > q[s[1], u1]
    assert (bits32(cb.download()) == bits32(k.c)).all()
    cb.close()


@pytest.mark.gpu
def test_posterior_at_the_ends_of_sigma2_on_a_map(E, eng):
    """16x8 at sigma2 = 1e-30 and 1e30 with test_posterior_at_the_ends_of_sigma2's assertions.  At the small end only the
    nearest units survive: the samples that equal a duplicated pair share the mass between its two units, which the
    replay gives as exact halves"""
    k = map_case(*MAPS[0])
    (u1, v1), (u2, v2) = k.pairs
    cb = on_map(E, eng, k)
    got, p = TR.check_the_ends_of_sigma2(E, eng, k.c, k.cl, k.x, k.dl, N_DATA, MAPS[0], cb)
    want = np.zeros((4, k.units))
    want[1, [u1, v1]] = -0.5                                           # sample 0: t = P = 1/2 on both units, q = 0
    want[2, [u2, v2]] = 0.5, -0.5
    want[3, [u2, v2]] = -0.5, 0.5
    other = ~p["own"][:4]                                              # (sample 1's class has a nearest unit of its own: q = 1 there)
    assert (p["q"][:4][other] == want[other]).all() and (p["q"][[0, 2, 3]] == want[[0, 2, 3]]).all()
    assert (p["pown"][[0, 1]] == [1.0, 0.0]).all() and np.allclose(p["pown"][[2, 3]], 0.5, rtol=1e-15, atol=0)
    q = got["q"][:4, :k.units]
    pair = np.zeros((4, k.units), dtype=bool)
    pair[:2, [u1, v1]] = True
    pair[2:, [u2, v2]] = True
    assert (q[other & ~pair] == 0).all() and (q[[0, 2, 3]][~pair[[0, 2, 3]]] == 0).all()
    assert bits64(q[1, u1]) == bits64(q[1, v1]) and q[1, u1] < 0 and bits64(q[0, u1]) == bits64(q[0, v1])
    assert q[2, u2] == -q[2, v2] > 0 and q[3, v2] == -q[3, u2] > 0
    assert list(got["correct"][:4]) == [1, 0, 1, 0]
    assert (bits32(cb.download()) == bits32(k.c)).all()
    cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_update_on_a_map(E, eng, xdim, ydim, dim):
    """rslvq_update from host sums indexed by unit, c different on every unit: the rows (downloaded in unit order) equal
    the float64 replay bit for bit and meet the np.longdouble allowance; every unit has moved; twice"""
    k = map_case(xdim, ydim, dim)
    rs = np.random.RandomState(k.units + 7 * dim)
    G, cc = rs.standard_normal((k.units, dim)) * 30, rs.standard_normal(k.units) * 10
    assert len(np.unique(cc)) == k.units and len(np.unique(G[:, 0])) == k.units
    alpha_t, sigma2, n = R.alpha_at(7.5, 9, 2), 0.7, 123
    want = R.update(k.c, G, cc, alpha_t, sigma2, n)
    wl, bound = R.update_longdouble(k.c, G, cc, alpha_t, sigma2, n)
    cb = on_map(E, eng, k)
    for again in range(2):
        cb.upload(k.c)
        E.rslvq_update(cb, alpha_t, sigma2, n, G, cc)
        after = cb.download()
        assert (bits32(after) == bits32(want)).all(), np.argwhere(bits32(after) != bits32(want))[:5]
        err = np.abs(after.astype(np.longdouble) - wl)
        assert (err <= bound).all(), float((err / bound).max())
        assert (bits32(after) != bits32(k.c)).any(axis=1).all()
    print("rslvq update on a map", (xdim, ydim, dim), "largest difference / bound:", float((err / bound).max()))
    cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_sums_on_a_map_do_not_read_storage(E, eng, xdim, ydim, dim):
    """rslvq_sums on a caller's Q (columns by unit) gives on the map the bits it gives on the same rows without a lattice,
    at chunk 64 and at the rule's, over a plain and a wrapped range, within the combine bound: the kernel reads the data
    and Q alone"""
    k = map_case(xdim, ydim, dim)
    q = TR.random_q(k.units + dim, N_DATA, k.units)
    ds = E.Dataset(eng, k.x, labels=k.dl)
    cb, plain = on_map(E, eng, k), E.Codebook(eng, k.c, labels=k.cl)
    for first in (0, N_DATA - 2):
        G, cc = E.rslvq_sums(cb, ds, q, first, N_DATA, chunk=64)
        for book, chunk in ((cb, 0), (plain, 64), (plain, 0)):
            G2, cc2 = E.rslvq_sums(book, ds, q, first, N_DATA, chunk=chunk)
            assert (bits64(G2) == bits64(G)).all() and (bits64(cc2) == bits64(cc)).all(), (first, book is cb, chunk)
        wG, wc, bG, bc = R.sums_longdouble(q, k.x, first)
        eG, ec = np.abs(G - wG).astype(f64), np.abs(cc - wc).astype(f64)
        print("rslvq sums on a map", (xdim, ydim, dim, first), "largest difference / bound:", float((eG / bG).max()), float((ec / bc).max()))
        assert (eG <= bG).all() and (ec <= bc).all(), (float((eG / bG).max()), float((ec / bc).max()))
    cb.close(); plain.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,dim", MAPS)
def test_whole_runs_on_a_map(E, eng, xdim, ydim, dim):
    """three epochs of rslvq_train over a wrapped range from the map (twice), from the same rows without a lattice and as
    test_rslvq.stage_epoch compositions at the rule's chunk and at chunk 64: rows, cost and correct by bit pattern; against
    the replay with test_runs' allowances; rslvq_search afterwards reports what an epoch at alpha 0 reports"""
    k = map_case(xdim, ydim, dim)
    sigma2, n = float(dim), N_DATA
    ds = E.Dataset(eng, k.x, labels=k.dl)
    cb = on_map(E, eng, k)
    cost, correct = E.rslvq_train(cb, ds, T, ALPHA, sigma2, first=FIRST, n=n)
    one = cb.download()
    cb.close()
    assert (bits32(one) != bits32(k.c)).any()
    for book in (on_map(E, eng, k), E.Codebook(eng, k.c, labels=k.cl)):
        cost2, correct2 = E.rslvq_train(book, ds, T, ALPHA, sigma2, first=FIRST, n=n)
        assert (bits32(book.download()) == bits32(one)).all() and (bits64(cost2) == bits64(cost)).all() and (correct2 == correct).all()
        book.close()
    cb = on_map(E, eng, k)
    for chunk in (0, 64):
        cb.upload(k.c)
        for t in range(T):                                             # an epoch is its stages
            ct, rt = TR.stage_epoch(E, cb, ds, E.glvq_alpha(ALPHA, T, t), sigma2, FIRST, n, chunk)
            assert bits64(ct)[()] == bits64(cost)[t] and rt == correct[t], (chunk, t)
        assert (bits32(cb.download()) == bits32(one)).all(), chunk
    scost, scorrect, spown = E.rslvq_search(cb, ds, sigma2, FIRST, n)
    p = E.rslvq_posterior(cb, ds, sigma2, FIRST, n)
    assert (bits64(spown) == bits64(p["pown"])).all() and scorrect == int(p["correct"].sum())
    ct, rt = E.rslvq_train(cb, ds, T, 0.0, sigma2, start_epoch=0, count=1, first=FIRST, n=n)     # alpha 0: the figures, no step
    assert bits64(scost) == bits64(ct)[0] and scorrect == rt[0] and (bits32(cb.download()) == bits32(one)).all()
    rows, rcost, rcorrect = R.train(k.c, k.cl, k.x, k.dl, T, ALPHA, sigma2, FIRST, n)
    print("rslvq runs on a map", (xdim, ydim, dim), "largest row difference:", float(np.abs(one - rows).max()), "cost, relative:",
          float(np.abs(cost / rcost - 1).max()))
    assert np.allclose(one, rows, rtol=0, atol=1e-5) and np.allclose(cost, rcost, rtol=1e-9, atol=0) and (correct == rcorrect).all()
    cb.close(); ds.close()


@pytest.mark.gpu
def test_the_tool_keeps_the_map_header_and_writes_the_engines_rows(E, eng, tools, tmp_path):
    """rslvq for two epochs on a labelled 16x8 hexa map written by textio.write_entries: the output keeps topology,
    neighbourhood and sides, its labels, and holds the rows engine.rslvq_train leaves for the same call on the map"""
    from som_lvq_pak_amd import textio
    k = copy.copy(map_case(*MAPS[0]))
    k.c = (np.round(k.c * 16) / 16).astype(f32)                        # values that "%g" keeps; the duplicates stay duplicates
    names = ["ape", "bee", "cat", "dog", "eel", "fox"]
    dat, cod, out = tmp_path / "d.dat", tmp_path / "m.cod", tmp_path / "o.cod"
    TR.write_dat(dat, k.x, k.dl, names)
    tab = textio.LabelTable()
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = k.dim, L.HEXA, L.BUBBLE, k.xdim, k.ydim, k.c
    m.labels = [[tab.to_index(names[int(l)])] for l in k.cl]
    textio.write_entries(str(cod), m, tab)
    assert (bits32(textio.read_entries(str(cod))[0].points) == bits32(k.c)).all()
    p = run("rslvq", "-din", dat, "-cin", cod, "-cout", out, "-epochs", 2, "-alpha", 2.5, "-sigma2", 1.5)
    assert p.returncode == 0, p.stderr
    ds = E.Dataset(eng, k.x, labels=k.dl)
    cb = on_map(E, eng, k, k.c)
    E.rslvq_train(cb, ds, 2, 2.5, 1.5)
    rows = cb.download()
    cb.close(); ds.close()
    assert (bits32(rows) != bits32(k.c)).any()
    head = [ln for ln in out.read_text().split("\n") if ln.strip() and not ln.startswith("#")][0]
    assert head.split() == [str(k.dim), "hexa", "16", "8", "bubble"], head
    tab2 = textio.LabelTable()
    got = textio.read_entries(str(out), tab2)[0]
    assert (got.dim, got.topol, got.neigh, got.xdim, got.ydim) == (k.dim, L.HEXA, L.BUBBLE, 16, 8)
    assert [tab2.names[ls[0]] for ls in got.labels] == [names[int(l)] for l in k.cl]
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in rows], dtype=f32)     # the file is "%g" text
    assert (bits32(got.points) == bits32(printed)).all(), np.argwhere(bits32(got.points) != bits32(printed))[:5]
