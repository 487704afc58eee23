"""numpy restatement of LVQ_PAK's med_distances and deviations (lvq_rout.c:384-491, 918-1004) and of the text mindist and
stddev print (mindist.c:95-106, stddev.c:74-80), bit for bit: the witness the GPU tests compare against.

Every operation carries the type C gives it in the reference (float = np.float32, each operation rounded on its own;
the reference is built with -ffp-contract=off):

    vector_dist_euc (lvq_pak.c:291-316)  components in order; masked in EITHER entry: skipped and counted;
                                         diff = a - b; sum += diff * diff        (sub, mul, add: three roundings)
                                         all dim skipped: -1, else (float) sqrt((double) sum)
    med_distances                        per entry the smallest distance to a LATER entry of its class (`dist < dissf`
                                         from FLT_MAX), per class the sorted values' [not / 2]; classes in add_hit order
    deviations                           per class float column sums in entry order (the entry's masked components
                                         skipped), / (float) noe; devdist per entry over ALL components, summed per class
                                         in entry order; (float) sqrt((double) (devs / (float) noe))

tests/test_classdist.py checks this file against outputs of the real reference (tests/golden/classdist, written by
tests/golden/make_golden_classdist.py), so the table above is pinned by the reference.

Also here: the generators of the test inputs that are not stored as fixtures.
"""
import os

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------ the nearest later entry of the same class
def nearest_later(rows, labels, mask=None):
    """(min_sq, state) as include/somhip.h somhip_class_nearest_later defines them: per row the smallest fp32 sum over
    the later rows of its label (+inf where none is finite), and 0 = no later row, 1 = valid, 2 = a later row of the
    label shares no unmasked component with the row.  (Under state 2 min_sq is not defined; here it is the minimum
    over all later rows, the empty sums +0 included.)"""
    rows = np.ascontiguousarray(rows, dtype=f32)
    labels = np.asarray(labels)
    n, dim = rows.shape
    min_sq = np.full(n, np.inf, dtype=f32)
    state = np.zeros(n, dtype=np.int32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for lab in np.unique(labels):
            idx = np.nonzero(labels == lab)[0]                # ascending: the order of the entries
            m = len(idx)
            if m < 2:
                continue
            X = rows[idx]
            M = None if mask is None else np.asarray(mask)[idx].astype(bool)
            acc = np.zeros((m, m), dtype=f32)
            skipped = np.zeros((m, m), dtype=np.int32)
            for i in range(dim):
                c = X[:, i]
                diff = c[None, :] - c[:, None]
                t = acc + diff * diff
                if M is None:
                    acc = t
                else:
                    skip = M[:, i][:, None] | M[:, i][None, :]
                    acc = np.where(skip, acc, t)
                    skipped += skip
            later = np.triu(np.ones((m, m), dtype=bool), 1)
            finite = later & np.isfinite(acc)
            best = np.where(finite, acc, f32(np.inf)).min(axis=1)
            empty = (later & (skipped == dim)).any(axis=1)
            has_later = np.arange(m) < m - 1
            min_sq[idx] = np.where(has_later, best, f32(np.inf))
            state[idx] = np.where(has_later, np.where(empty, 2, 1), 0)
    return min_sq, state


def add_hit_order(labels):
    """[(label, freq)] as a hit list holds them after add_hit of every label in order (labels.c:370-407): a new label
    goes last, a label moves up while its predecessor has a strictly smaller count"""
    lab, freq = [], []
    for x in labels:
        x = int(x)
        if x not in lab:
            lab.append(x)
            freq.append(1)
            continue
        i = lab.index(x)
        freq[i] += 1
        while i > 0 and freq[i - 1] < freq[i]:
            lab[i - 1], lab[i] = lab[i], lab[i - 1]
            freq[i - 1], freq[i] = freq[i], freq[i - 1]
            i -= 1
    return list(zip(lab, freq))


def distances_from(min_sq, state):
    """dissf of every row with a later one: -1 under state 2, FLT_MAX where nothing finite was met, else the root"""
    d = np.sqrt(min_sq.astype(f64)).astype(f32)
    d = np.where(np.isinf(min_sq), FLT_MAX, d)
    return np.where(state == 2, f32(-1.0), d).astype(f32)


def med_distances(rows, labels, mask=None, nearest=None):
    """[(label, noe, median)] in add_hit order; nearest = (min_sq, state) from elsewhere (the engine) or None"""
    labels = np.asarray(labels)
    min_sq, state = nearest if nearest is not None else nearest_later(rows, labels, mask)
    dist = distances_from(min_sq, state)
    out = []
    for lab, noe in add_hit_order(labels):
        vals = np.sort(dist[(labels == lab) & (state != 0)])
        out.append((lab, noe, f32(vals[len(vals) // 2]) if len(vals) else f32(0.0)))
    return out


def deviations(rows, labels, mask, md):
    """devs per class of md = [(label, noe, ...)]; raises KeyError(label) for a label md has no class for"""
    rows = np.ascontiguousarray(rows, dtype=f32)
    labels = np.asarray(labels)
    n, dim = rows.shape
    cls = {lab: i for i, (lab, _, _) in enumerate(md)}
    noe = [f32(m[1]) for m in md]
    avers = np.zeros((len(md), dim), dtype=f32)
    which = np.empty(n, dtype=np.int64)
    for r in range(n):
        which[r] = cls[int(labels[r])]
        if mask is None:
            avers[which[r]] = avers[which[r]] + rows[r]
        else:
            avers[which[r]] = np.where(mask[r] != 0, avers[which[r]], avers[which[r]] + rows[r])
    for i in range(len(md)):
        avers[i] = avers[i] / noe[i]
    d = np.zeros(n, dtype=f32)
    for j in range(dim):
        diff = rows[:, j] - avers[which, j]
        d = d + diff * diff
    devs = np.zeros(len(md), dtype=f32)
    for r in range(n):
        devs[which[r]] = devs[which[r]] + d[r]
    return [f32(np.sqrt(f64(devs[i] / noe[i]))) for i in range(len(md))]


def report(md, devs, names, word):
    """the text of mindist (word 'min') / stddev (word 'med'); devs None: mindist without -din"""
    out = ""
    for i, (lab, noe, dist) in enumerate(md):
        out += "In class %9s %3d units, %s dist.: %6.3f" % (names[lab], noe, word, float(dist))
        out += "\n" if devs is None else ", stand. dev.: %6.3f \n" % float(devs[i])
    return out


# ------------------------------------------------------------------ generated inputs (not stored: md5 in expected.json)
GENERATED = ("ex1_noF.dat", "scaled.dat", "masked.dat")


def scaled_case():
    """301 rows, dim 5, classes of 1, 2, 63, 100 and 135 rows shuffled together, one duplicated row, components about
    N(0, 40000^2): the nearest distances land in [2^14, 2^24), where %6.3f prints adjacent floats differently"""
    rs = np.random.RandomState(20240611)
    sizes = (1, 2, 63, 100, 135)
    labels = np.concatenate([np.full(s, k, dtype=np.int64) for k, s in enumerate(sizes)])
    rs.shuffle(labels)
    rows = (40000.0 * rs.standard_normal((len(labels), 5))).astype(f32)
    members = np.nonzero(labels == 3)[0]
    rows[members[40]] = rows[members[7]]
    return rows, labels, ["s1", "s2", "s63", "s100", "s135"]


MASKED_TEXT = """4
# the two rows of class R share no unmasked component, nor do the first two of P; the fully masked row is dropped on load
1.5 2.25 x x P
0.5 x 3 4 Q
x x 3.5 4.75 P
2 2 3 3 P
x x x x Q
0.25 1 x 3.5 Q
1.75 x 2.5 x P
x 1.5 3.25 3 Q
3 x x 1 R
x 2.75 1.5 x R
0.75 x 3 x Q
"""


def write_generated(directory, data_dir):
    """writes GENERATED into `directory` (ex1.dat is read from data_dir)"""
    with open(os.path.join(data_dir, "ex1.dat")) as f:
        lines = f.read().split("\n")
    kept = [ln for ln in lines if not ln.endswith(" F")]
    assert len(kept) == len(lines) - 1
    with open(os.path.join(directory, "ex1_noF.dat"), "w") as f:
        f.write("\n".join(kept))
    rows, labels, names = scaled_case()
    with open(os.path.join(directory, "scaled.dat"), "w") as f:
        f.write("5\n")
        for r in range(rows.shape[0]):
            f.write(" ".join("%.9g" % float(v) for v in rows[r]) + " " + names[labels[r]] + "\n")
    with open(os.path.join(directory, "masked.dat"), "w") as f:
        f.write(MASKED_TEXT)
