"""Python host mirror of the engine's C ABI (include/somhip.h): thin objects over ctypes,
numpy in / numpy out.  Used by the parity tests and bench.py; the command-line tools are
C (som_lvq_pak_amd/host/).  Everything here runs on the GPU through libsomhip.so -- there
is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LvqParams, SomParams, check

TOPOL_HEXA, TOPOL_RECT, TOPOL_LVQ = 3, 4, 2
NEIGH_BUBBLE, NEIGH_GAUSSIAN = 1, 2
ALPHA_LINEAR, ALPHA_INVERSE_T = 1, 2
LVQ1, OLVQ1, LVQ2, LVQ3 = 1, 2, 3, 4
TIE_FIRST, TIE_KNN = 0, 1
UMAT_AVERAGE, UMAT_MEDIAN = 1, 2


def __getattr__(name):
    if name == "KNN_MAX":                   # most neighbours find_winners takes: asked of the library, when first wanted
        return _lib.load().somhip_knn_max()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def _p(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


class Engine:
    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.somhip_engine_create(device, C.byref(h)))
        self.h = h
        self.device = device
        self._children = []          # weakrefs: mirrors must be destroyed before their engine

    def _adopt(self, child):
        import weakref
        self._children.append(weakref.ref(child))

    def close(self):
        if self.h:
            for ref in self._children:
                child = ref()
                if child is not None:
                    child.close()
            self._children = []
            self.lib.somhip_engine_destroy(self.h)
            self.h = None

    def sync(self):
        check(self.lib.somhip_engine_sync(self.h))

    @property
    def stream(self):
        return self.lib.somhip_engine_stream(self.h)

    def set_scan_mode(self, mode):
        """'direct', 'mfma' or 'mfma_bf16' (see include/somhip.h)"""
        check(self.lib.somhip_engine_set_scan_mode(self.h, {"direct": 0, "mfma": 1, "mfma_bf16": 2}[mode]))

    def set_update_mode(self, mode):
        """'exact' (adapt_vector's arithmetic, bit-identical to the batch oracle) or 'gemm' (matrix-pipe form)"""
        check(self.lib.somhip_engine_set_update_mode(self.h, {"exact": 0, "gemm": 1}[mode]))

    def scan_stats(self):
        out = (C.c_uint64 * 8)()
        check(self.lib.somhip_scan_stats(self.h, out))
        return {"groups": out[0], "rows": out[1], "max_groups_per_sample": out[2], "samples": out[3],
                "row_updates": out[4], "group_updates": out[5], "gemm_entries": out[6], "l2_pairs": out[7]}

    def lvq_stats(self):
        """exact batched LVQ: codebook rescans (batches) and samples so far"""
        out = (C.c_uint64 * 12)()
        check(self.lib.somhip_lvq_stats(self.h, out))
        return {"batches": out[0], "samples": out[1], "stop_list": out[2], "stop_cache": out[3],
                "phase_us": [out[4 + k] / 100.0 for k in range(4)], "components": out[8], "largest": out[9],
                "topk_pairs": out[10], "topk_overflow": out[11]}

    # --- timing table (HIP events on the engine's stream) ---
    def timing(self, on=True):
        check(self.lib.somhip_timing_enable(self.h, int(on)))

    def timing_select(self, names=None):
        """time only the named kernels (None = all): fewer HIP events on the stream"""
        mask = 0
        for i in range(self.lib.somhip_kernel_count()):
            if names is None or self.lib.somhip_kernel_name(i).decode() in names:
                mask |= 1 << i
        check(self.lib.somhip_timing_select(self.h, mask))

    def timing_reset(self):
        check(self.lib.somhip_timing_reset(self.h))

    def timing_table(self):
        out = {}
        for i in range(self.lib.somhip_kernel_count()):
            n = C.c_int64(0)
            ms = C.c_double(0)
            check(self.lib.somhip_timing_get(self.h, i, C.byref(n), C.byref(ms)))
            out[self.lib.somhip_kernel_name(i).decode()] = (n.value, ms.value)
        return out

    def mapset_timing(self):
        """(launches, ms) of the map-set kernels while timing is on (somhip_mapset_timing; they are not in timing_table)"""
        n = (C.c_int64 * 2)()
        ms = (C.c_double * 2)()
        check(self.lib.somhip_mapset_timing(self.h, n, ms))
        return {"k_mapset_train": (n[0], ms[0]), "k_mapset_winners": (n[1], ms[1])}

    def knn_timing(self):
        """(launches, ms) of the wide k-NN route's two stages while timing is on (somhip_knn_timing; they are not in
        timing_table): one launch of each per chunk of samples"""
        n = (C.c_int64 * 2)()
        ms = (C.c_double * 2)()
        check(self.lib.somhip_knn_timing(self.h, n, ms))
        return {"k_knn_dist": (n[0], ms[0]), "k_knn_select": (n[1], ms[1])}

    def knn_vote_timing(self):
        """(launches, ms) of k_knn_vote while timing is on (somhip_knn_vote_timing; it is not in timing_table): one launch
        per chunk of samples"""
        n = C.c_int64(0)
        ms = C.c_double(0)
        check(self.lib.somhip_knn_vote_timing(self.h, C.byref(n), C.byref(ms)))
        return {"k_knn_vote": (n.value, ms.value)}

    def map_quality_timing(self):
        """(launches, ms) of map_quality's two kernels while timing is on (somhip_map_quality_timing; they are not in
        timing_table): one launch of each per chunk of samples"""
        n = (C.c_int64 * 2)()
        ms = (C.c_double * 2)()
        check(self.lib.somhip_map_quality_timing(self.h, n, ms))
        return {"k_quality_pairs": (n[0], ms[0]), "k_quality_units": (n[1], ms[1])}

    def conn_timing(self):
        """(launches, ms) of map_connectivity's pair passes while timing is on (somhip_conn_timing; they are not in
        timing_table): the key pass once per chunk of samples; per slab the sort once, the run pass and the merge three
        timed scopes each (two kernels around a scan)"""
        n = (C.c_int64 * 4)()
        ms = (C.c_double * 4)()
        check(self.lib.somhip_conn_timing(self.h, n, ms))
        return {"k_conn_keys": (n[0], ms[0]), "sort": (n[1], ms[1]), "runs": (n[2], ms[2]), "merge": (n[3], ms[3])}

    def batchmap_timing(self):
        """(launches, ms) of the batch map's stages while timing is on (somhip_batchmap_timing; they are not in
        timing_table): group = the winners pass per chunk, the scan of the counts and the sort by winner"""
        n = (C.c_int64 * 3)()
        ms = (C.c_double * 3)()
        check(self.lib.somhip_batchmap_timing(self.h, n, ms))
        return {"group": (n[0], ms[0]), "k_batchmap_sums": (n[1], ms[1]), "k_batchmap_combine": (n[2], ms[2])}

    def glvq_timing(self):
        """(launches, ms) of batch GLVQ's stages while timing is on (somhip_glvq_timing; they are not in timing_table):
        search = the class-wise scan per chunk, or one span around the list route's top-8 search, pick and remainder;
        terms = k_glvq_terms, the scans of the counts and the sorts by winner"""
        n = (C.c_int64 * 4)()
        ms = (C.c_double * 4)()
        check(self.lib.somhip_glvq_timing(self.h, n, ms))
        return {"search": (n[0], ms[0]), "terms": (n[1], ms[1]), "k_glvq_sums": (n[2], ms[2]), "k_glvq_update": (n[3], ms[3])}

    def ng_timing(self):
        """(launches, ms) of batch neural gas's stages while timing is on (somhip_ng_timing; they are not in timing_table):
        group = k_ng_entries per chunk, the scan of the counts and the sort by unit, once per segment.  The search counts
        under its own kernels (timing_table, knn_timing)."""
        n = (C.c_int64 * 3)()
        ms = (C.c_double * 3)()
        check(self.lib.somhip_ng_timing(self.h, n, ms))
        return {"group": (n[0], ms[0]), "k_ng_sums": (n[1], ms[1]), "k_ng_update": (n[2], ms[2])}

    def ng_dense_timing(self):
        """(launches, ms) of dense batch neural gas's stages while timing is on (somhip_ng_dense_timing; they are not in
        timing_table and not under timing_select): distances = the sample tiles and k_knn_dist, one span per chunk; sums =
        k_rslvq_sums.  The update counts under ng_timing's k_ng_update."""
        n = (C.c_int64 * 3)()
        ms = (C.c_double * 3)()
        check(self.lib.somhip_ng_dense_timing(self.h, n, ms))
        return {"distances": (n[0], ms[0]), "k_ng_dense_weights": (n[1], ms[1]), "sums": (n[2], ms[2])}

    def grlvq_timing(self):
        """(launches, ms) of batch GRLVQ's stages while timing is on (somhip_grlvq_timing; they are not in timing_table):
        search = the weighted class-wise scan per chunk; terms = batch GLVQ's stage, counted under its id (glvq_timing
        reports the same figures)"""
        n = (C.c_int64 * 5)()
        ms = (C.c_double * 5)()
        check(self.lib.somhip_grlvq_timing(self.h, n, ms))
        return {"search": (n[0], ms[0]), "terms": (n[1], ms[1]), "k_grlvq_sums": (n[2], ms[2]), "k_grlvq_relevance": (n[3], ms[3]),
                "k_grlvq_update": (n[4], ms[4])}

    def gmlvq_timing(self):
        """(launches, ms) of batch GMLVQ's stages while timing is on (somhip_gmlvq_timing; they are not in timing_table):
        project = the projections of the samples and of the rows; search, terms, sums = batch GLVQ's stages, counted under
        its ids (glvq_timing reports the same figures); k_gmlvq_omega_grad = the gradient of omega with its reduction"""
        n = (C.c_int64 * 6)()
        ms = (C.c_double * 6)()
        check(self.lib.somhip_gmlvq_timing(self.h, n, ms))
        return {"k_gmlvq_project": (n[0], ms[0]), "search": (n[1], ms[1]), "terms": (n[2], ms[2]), "sums": (n[3], ms[3]),
                "k_gmlvq_omega_grad": (n[4], ms[4]), "k_gmlvq_update": (n[5], ms[5])}

    def rslvq_timing(self):
        """(launches, ms) of batch RSLVQ's stages while timing is on (somhip_rslvq_timing; they are not in timing_table
        and not under timing_select): distances = the sample tiles and k_knn_dist, one span per chunk"""
        n = (C.c_int64 * 4)()
        ms = (C.c_double * 4)()
        check(self.lib.somhip_rslvq_timing(self.h, n, ms))
        return {"distances": (n[0], ms[0]), "k_rslvq_posterior": (n[1], ms[1]), "k_rslvq_sums": (n[2], ms[2]),
                "k_rslvq_update": (n[3], ms[3])}

    def distortion_timing(self):
        """(launches, ms) of map distortion's stages while timing is on (somhip_distortion_timing; they are not in
        timing_table): group = the winners pass per chunk, the scan of the counts and the sort by winner; sums = the
        continued sums and the two Q passes; evaluate = the gaussian table, the kernel and the two fold passes"""
        n = (C.c_int64 * 3)()
        ms = (C.c_double * 3)()
        check(self.lib.somhip_distortion_timing(self.h, n, ms))
        return {"group": (n[0], ms[0]), "sums": (n[1], ms[1]), "evaluate": (n[2], ms[2])}

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        check(self.lib.somhip_device_alloc(self.h, nbytes, C.byref(p)))
        return p

    def device_free(self, p):
        check(self.lib.somhip_device_free(self.h, p))

    def copy_to_host(self, addr, nbytes):
        """uint8[nbytes] from device address addr (somhip_copy_to_host)"""
        out = np.empty(nbytes, dtype=np.uint8)
        check(self.lib.somhip_copy_to_host(self.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(addr), nbytes))
        return out

    def copy_to_device(self, addr, data):
        """the bytes of the array `data` to device address addr (somhip_copy_to_device)"""
        data = np.ascontiguousarray(data)
        check(self.lib.somhip_copy_to_device(self.h, C.c_void_p(addr), data.ctypes.data_as(C.c_void_p), data.nbytes))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_units(xdim, ydim, shard_index, shard_count, lib=None):
    """Global unit indices of the rows of interleaved shard `shard_index` of `shard_count` (somhip_shard_units)."""
    lib = lib or _lib.load()
    n = C.c_int64()
    check(lib.somhip_shard_units(xdim, ydim, shard_index, shard_count, None, C.byref(n)))
    units = np.empty(n.value, dtype=np.int64)
    check(lib.somhip_shard_units(xdim, ydim, shard_index, shard_count, _p(units, _lib.c_i64_p), C.byref(n)))
    return units


class Codebook:
    """Device mirror of the `codes` list (reference lvq_pak.h:89-113)."""

    def __init__(self, engine, rows, topol=TOPOL_LVQ, neigh=0, xdim=0, ydim=0, labels=None,
                 row_offset=0, n_global=None, interleave=None):
        """interleave=(shard_index, shard_count): `rows` are the units shard_units(...) lists, in that order
        (somhip_codebook_create_interleaved); otherwise the contiguous rows [row_offset, row_offset + n)."""
        self.e = engine
        rows = _arr(rows, np.float32)
        self.n, self.dim = rows.shape
        labels = _arr(labels, np.int32)
        self.labels = labels
        self.topol, self.neigh, self.xdim, self.ydim = topol, neigh, xdim, ydim
        self.row_offset = row_offset
        self.n_global = self.n if n_global is None else n_global
        h = C.c_void_p()
        self.interleave = interleave
        if interleave is not None:
            self.n_global = xdim * ydim
            check(engine.lib.somhip_codebook_create_interleaved(engine.h, _p(rows, _lib.c_float_p), self.n, self.dim,
                                                                topol, neigh, xdim, ydim, interleave[0],
                                                                interleave[1], C.byref(h)))
        else:
            check(engine.lib.somhip_codebook_create(engine.h, _p(rows, _lib.c_float_p), _p(labels, _lib.c_i32_p),
                                                    self.n, self.dim, topol, neigh, xdim, ydim, row_offset,
                                                    self.n_global, C.byref(h)))
        self.h = h
        engine._adopt(self)

    def download(self):
        out = np.empty((self.n, self.dim), dtype=np.float32)
        check(self.e.lib.somhip_codebook_download(self.h, _p(out, _lib.c_float_p)))
        return out

    def upload(self, rows):
        rows = _arr(rows, np.float32)
        assert rows.shape == (self.n, self.dim)
        check(self.e.lib.somhip_codebook_upload(self.h, _p(rows, _lib.c_float_p)))

    def close(self):
        if self.h and self.e.h:
            self.e.lib.somhip_codebook_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dataset:
    """Device mirror of the `data` list (one -buffer worth of rows)."""

    def __init__(self, engine, rows=None, mask=None, labels=None, weight=None, fixed_xy=None,
                 device_ptr=None, n=None, dim=None, generate=None):
        """generate=(seed, k_centres, dim, first_row, n_rows): the seeded mixture stream made in HBM
        (somhip_dataset_generate); self.centres then holds each row's mixture id."""
        self.e = engine
        h = C.c_void_p()
        if generate is not None:
            seed, k, gdim, first, gn = generate
            self.n, self.dim = gn, gdim
            self.centres = np.empty(gn, dtype=np.int32)
            check(engine.lib.somhip_dataset_generate(engine.h, seed, k, gdim, first, gn,
                                                     _p(self.centres, _lib.c_i32_p), C.byref(h)))
        elif device_ptr is not None:
            self.n, self.dim = n, dim
            check(engine.lib.somhip_dataset_wrap_device(engine.h, C.c_void_p(device_ptr), n, dim, C.byref(h)))
        else:
            rows = _arr(rows, np.float32)
            self.n, self.dim = rows.shape
            mask = _arr(mask, np.uint8)
            labels = _arr(labels, np.int32)
            weight = _arr(weight, np.int16)
            fixed_xy = _arr(fixed_xy, np.int16)
            check(engine.lib.somhip_dataset_create(engine.h, _p(rows, _lib.c_float_p), self.n, self.dim,
                                                   _p(mask, _lib.c_u8_p), _p(labels, _lib.c_i32_p),
                                                   _p(weight, _lib.c_i16_p), _p(fixed_xy, _lib.c_i16_p),
                                                   C.byref(h)))
        self.h = h
        engine._adopt(self)

    def rows(self, first, count):
        """host copy of rows [first, first + count) (somhip_dataset_download_rows)"""
        out = np.empty((count, self.dim), dtype=np.float32)
        check(self.e.lib.somhip_dataset_download_rows(self.h, first, count, _p(out, _lib.c_float_p)))
        return out

    def close(self):
        if self.h and self.e.h:
            self.e.lib.somhip_dataset_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gen_rows(seed, k_centres, dim, first_row, n_rows):
    """Host form of the seeded mixture stream (numpy restatement of pak_gen_row / k_gen_mixture): (rows, centres)."""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)

    def mix(x):
        with np.errstate(over="ignore"):
            x = (x + np.uint64(0x9E3779B97F4A7C15)) & M
            x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M
            x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M
            return x ^ (x >> np.uint64(31))

    def z(sd, counter):
        total = np.zeros(counter.shape, dtype=np.int64)
        with np.errstate(over="ignore"):
            for w in range(3):
                v = mix(np.uint64(sd) ^ (np.uint64(3) * counter + np.uint64(w)))
                for sh in (0, 16, 32, 48):
                    total += ((v >> np.uint64(sh)) & np.uint64(0xFFFF)).astype(np.int64)
        return ((total - 6 * 65535).astype(np.float32) / np.float32(65536.0)).astype(np.float32)

    rows = np.arange(first_row, first_row + n_rows, dtype=np.uint64)
    cen = (mix(np.uint64(seed ^ 0xB492B66FBE98F273) ^ rows) % np.uint64(k_centres)).astype(np.int64)
    cols = np.arange(dim, dtype=np.uint64)[None, :]
    mu = np.float32(4.0) * z(seed ^ 0xC3A5C85C97CB3127, cen.astype(np.uint64)[:, None] * np.uint64(dim) + cols)
    x = mu + z(seed, rows[:, None] * np.uint64(dim) + cols)
    return x.astype(np.float32), cen.astype(np.int32)


def column_minmax(ds):
    """Per-component (lo, hi, count) of the unmasked data on the device (somhip_column_minmax)."""
    lo = np.empty(ds.dim, dtype=np.float32)
    hi = np.empty(ds.dim, dtype=np.float32)
    cnt = np.empty(ds.dim, dtype=np.int64)
    check(ds.e.lib.somhip_column_minmax(ds.h, _p(lo, _lib.c_float_p), _p(hi, _lib.c_float_p), _p(cnt, _lib.c_i64_p)))
    return lo, hi, cnt


def column_sums(ds):
    """lininit's first data pass (somhip_column_sums): per component the fp32 sum of the unmasked values, rows in
    order, and how many there are: (sum float32[dim], count int64[dim])."""
    s = np.empty(ds.dim, dtype=np.float32)
    cnt = np.empty(ds.dim, dtype=np.int64)
    check(ds.e.lib.somhip_column_sums(ds.h, _p(s, _lib.c_float_p), _p(cnt, _lib.c_i64_p)))
    return s, cnt


def centered_products(ds, mean):
    """lininit's second data pass (somhip_centered_products): R[i, j] = sum over the rows, in order and in fp32, of
    (x[r, i] - mean[i]) * (x[r, j] - mean[j]) where both components are unmasked.  float32[dim, dim] as the ABI
    returns it: j >= i filled, j < i left 0."""
    mean = _arr(mean, np.float32)
    assert mean.shape == (ds.dim,)
    r = np.empty((ds.dim, ds.dim), dtype=np.float32)
    check(ds.e.lib.somhip_centered_products(ds.h, _p(mean, _lib.c_float_p), _p(r, _lib.c_float_p)))
    return r


def orand_stream(seed, count):
    """The reference's LCG (lvq_pak.c:459-473: next = next * 23 % 100000001, value = next % 32767) as a numpy
    array of `count` draws after init_random(seed): state_k = seed * 23^k mod M, evaluated blockwise."""
    M = np.uint64(100000001)
    blk = 1 << 12
    pw = np.empty(blk, dtype=np.uint64)                 # 23^(i+1) mod M
    v = 1
    for i in range(blk):
        v = v * 23 % 100000001
        pw[i] = v
    nblk = (count + blk - 1) // blk
    base = np.empty(nblk, dtype=np.uint64)              # state before block j
    s = int(seed) % 100000001
    step = int(pw[-1])
    for j in range(nblk):
        base[j] = s
        s = s * step % 100000001
    st = (base[:, None] * pw[None, :]) % M
    return (st.reshape(-1)[:count] % np.uint64(32767)).astype(np.int64)


def randinit_from_bbox(lo, hi, cnt, xdim, ydim, seed):
    """randinit_codes (som_rout.c:98-150) from the data's bounding box: maximum seeded with FLT_MIN, minimum with
    FLT_MAX (:108-111), then unit by unit, component by component lo + (hi - lo) * ((float)orand() / 32768.0)
    evaluated in double and stored as float (:140-150); components without data get 0."""
    lo = np.minimum(np.asarray(lo, dtype=np.float32), np.float32(3.402823466e+38))
    hi = np.maximum(np.asarray(hi, dtype=np.float32), np.float32(1.17549435e-38))
    d = lo.shape[0]
    n = xdim * ydim
    r = orand_stream(seed, n * d).reshape(n, d).astype(np.float32).astype(np.float64) / 32768.0
    span = (hi - lo).astype(np.float32).astype(np.float64)
    out = (lo.astype(np.float64)[None, :] + span[None, :] * r).astype(np.float32)
    out[:, np.asarray(cnt) == 0] = 0.0
    return out


def find_winners(cb, ds, first=0, count=None, knn=1, tie=TIE_FIRST):
    """WINNER_FUNCTION over data rows [first, first+count): (index, diff, ret).

    knn 1..8 takes the top-k scans; knn 9..KNN_MAX (with TIE_KNN) the wide route: exact distances to every row, then a
    select per sample, in chunks of samples (scan_plan(cb, ds, count, knn)["chunk"]).
    Masked data sets (Dataset(..., mask=...)) work for every knn (1..KNN_MAX): only the sample's mask counts
    (lvq_pak.c:179-186); a sample with every component masked gives ret 0 and index -2."""
    count = ds.n if count is None else count
    idx = np.empty((count, knn), dtype=np.int32)
    diff = np.empty((count, knn), dtype=np.float32)
    ret = np.empty(count, dtype=np.int32)
    check(cb.e.lib.somhip_find_winners(cb.h, ds.h, first, count, knn, tie, _p(idx, _lib.c_i32_p),
                                       _p(diff, _lib.c_float_p), _p(ret, _lib.c_i32_p)))
    return idx, diff, ret


def knn_vote(cb, ds, first=0, count=None, knn=5):
    """The class vote of the knn nearest rows of data rows [first, first+count), formed on the device behind the search
    find_winners would run (somhip_knn_vote): (label, freq, own, found), int32 arrays of `count`.

    found: neighbours found (fewer than knn on a small codebook, 0 if every component of the sample is masked); label: the
    head of the reference's hit list over their labels, nearest first (-1 if found is 0); freq: its count; own: neighbours
    with the sample's own label (-1 for a Dataset without labels).  The codebook needs labels and must be a whole one."""
    count = ds.n if count is None else count
    out = [np.empty(count, dtype=np.int32) for _ in range(4)]
    check(cb.e.lib.somhip_knn_vote(cb.h, ds.h, first, count, knn, *[_p(a, _lib.c_i32_p) for a in out]))
    return tuple(out)


def map_quality(cb, ds, first=0, count=None, hits=None, qsum=None, qerror=0.0):
    """Topographic error and per-unit statistics of a map over data rows (first + s) % ds.n, s < count, formed on the
    device behind the top-2 search (somhip_map_quality): (totals, hits, qsum).

    totals: {"searched", "topo_defined", "topo_errors", "qerror"} -- the samples with an unmasked component, those with a
    second-best unit, those whose best and second-best units are not lattice neighbours, and find_qerror's float sum
    continued from `qerror`.  hits (uint32[cb.n]): samples won per unit; qsum (float64[cb.n]): the sum of their distances
    in data order.  Arrays passed in are not changed: the returned ones continue them, so a run cut into several calls
    (hits, qsum and totals["qerror"] handed on) gives the bits of one call."""
    count = ds.n if count is None else count
    hits = np.zeros(cb.n, dtype=np.uint32) if hits is None else np.array(hits, dtype=np.uint32)
    qsum = np.zeros(cb.n, dtype=np.float64) if qsum is None else np.array(qsum, dtype=np.float64)
    assert hits.shape == (cb.n,) and qsum.shape == (cb.n,)
    tot = _lib.QualityTotals()
    check(cb.e.lib.somhip_map_quality(cb.h, ds.h, first, count, _p(hits, _lib.c_u32_p), _p(qsum, _lib.c_double_p),
                                      float(np.float32(qerror)), C.byref(tot)))
    return ({"searched": tot.searched, "topo_defined": tot.topo_defined, "topo_errors": tot.topo_errors,
             "qerror": np.float32(tot.qerror)}, hits, qsum)


CONN_SLAB = 1 << 20      # somhip.h SOMHIP_CONN_SLAB: the samples whose pairs map_connectivity sorts at a time


class Conn:
    """A pair table on the device (somhip_conn): for every ordered pair (best unit, second-best unit) that some sample
    has, the number of such samples, ascending by pair.  map_connectivity adds to it; it lives until closed."""

    def __init__(self, engine):
        self.e = engine
        h = C.c_void_p()
        check(engine.lib.somhip_conn_create(engine.h, C.byref(h)))
        self.h = h
        engine._adopt(self)

    def clear(self):
        check(self.e.lib.somhip_conn_clear(self.h))

    def size(self):
        """(pairs, samples): the entries and the sum of their counts"""
        pairs, samples = C.c_int64(0), C.c_uint64(0)
        check(self.e.lib.somhip_conn_size(self.h, C.byref(pairs), C.byref(samples)))
        return pairs.value, samples.value

    def read(self, first=0, n=None):
        """(b1, b2, count) of entries [first, first + n) in table order: uint32, uint32, uint64 arrays"""
        n = self.size()[0] - first if n is None else n
        m = max(n, 0)
        b1, b2, count = np.empty(m, dtype=np.uint32), np.empty(m, dtype=np.uint32), np.empty(m, dtype=np.uint64)
        check(self.e.lib.somhip_conn_read(self.h, first, n, _p(b1, _lib.c_u32_p), _p(b2, _lib.c_u32_p), _p(count, _lib.c_u64_p)))
        return b1, b2, count

    def close(self):
        if self.h and self.e.h:
            self.e.lib.somhip_conn_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def map_connectivity(cb, ds, conn, first=0, count=None, quality=False, hits=None, qsum=None, qerror=0.0):
    """Adds to `conn`, per ordered pair (best unit, second-best unit), the samples of data rows (first + s) % ds.n,
    s < count, that have it (somhip_map_connectivity).  quality=False: returns None; any whole codebook, with a lattice or
    without.  quality=True: map_quality's (totals, hits, qsum) from the same search, with the same bits."""
    count = ds.n if count is None else count
    if not quality:
        assert hits is None and qsum is None
        check(cb.e.lib.somhip_map_connectivity(cb.h, ds.h, first, count, conn.h, None, None, 0.0, None))
        return None
    hits = np.zeros(cb.n, dtype=np.uint32) if hits is None else np.array(hits, dtype=np.uint32)
    qsum = np.zeros(cb.n, dtype=np.float64) if qsum is None else np.array(qsum, dtype=np.float64)
    assert hits.shape == (cb.n,) and qsum.shape == (cb.n,)
    tot = _lib.QualityTotals()
    check(cb.e.lib.somhip_map_connectivity(cb.h, ds.h, first, count, conn.h, _p(hits, _lib.c_u32_p), _p(qsum, _lib.c_double_p),
                                           float(np.float32(qerror)), C.byref(tot)))
    return ({"searched": tot.searched, "topo_defined": tot.topo_defined, "topo_errors": tot.topo_errors,
             "qerror": np.float32(tot.qerror)}, hits, qsum)


ROUTES = ("masked", "direct", "one_level", "two_level", "wide")


def scan_plan(cb, ds, count, want=1):
    """The plan of a winner search of `count` samples for the nearest row (want 1) or the top-k width `want` (2, 4, 8)
    (somhip_debug_scan_plan; host arithmetic, no GPU work): a dict of the route and the stage choices behind it.
    want 9..KNN_MAX (a knn of the wide route): {"route": "wide", "chunk": samples per chunk}."""
    out = (C.c_int32 * 8)()
    check(cb.e.lib.somhip_debug_scan_plan(cb.h, ds.h, count, want, out))
    if ROUTES[out[0]] == "wide":
        return {"route": "wide", "chunk": out[1]}
    return {"route": ROUTES[out[0]], "kth": out[1], "bf16": bool(out[2]), "l1_ring": bool(out[3]),
            "by_group": bool(out[4]), "l2_global": bool(out[5]), "fused_gmin": bool(out[6])}


def debug_prepared(cb, ds, first, count):
    """What the preparation of a nearest-row search of data rows [first, first + count) leaves on the device
    (somhip_debug_prepared; bf16 scan mode on a pre-filter route): a dict of numpy arrays, bf16 values as uint16;
    `rowmajor`, `xlo`, `xrow` and `tau1` are None where the search makes none."""
    d8 = (cb.dim + 7) // 8
    ng, nsb = (cb.n + 63) // 64, (count + 31) // 32
    out = {"chi": np.zeros((ng, d8, 64, 8), np.uint16), "clo": np.zeros((ng, d8, 64, 8), np.uint16),
           "cn": np.zeros(ng * 64, np.float32), "rowmajor": np.zeros((ng * 64, cb.dim), np.float32),
           "xhi": np.zeros((nsb, d8, 32, 8), np.uint16), "xlo": np.zeros((nsb, d8, 32, 8), np.uint16),
           "xrow": np.zeros((nsb * 32, d8, 2, 8), np.uint16), "tau": np.zeros(count, np.float32),
           "tau1": np.zeros(count, np.float32)}
    info = (C.c_int32 * 4)()
    u16, f32 = _lib.c_u16_p, _lib.c_float_p
    check(cb.e.lib.somhip_debug_prepared(cb.h, ds.h, first, count, _p(out["chi"], u16), _p(out["clo"], u16), _p(out["cn"], f32),
                                         _p(out["rowmajor"], f32), _p(out["xhi"], u16), _p(out["xlo"], u16),
                                         _p(out["xrow"], u16), _p(out["tau"], f32), _p(out["tau1"], f32), info))
    assert info[3] == d8
    if not info[0]:
        out["rowmajor"] = None
    if not info[1]:
        out["xlo"] = None
    if not info[2]:
        out["xrow"] = out["tau1"] = None
    return out


def debug_prepared_state(cb):
    """The codebook's cache of prepared copies as it lies on the device now (somhip_debug_prepared_state; nothing is
    launched, no flag changes): a dict of the flags prep_valid, rowmajor_valid, bm_open, bm_moved (ints) and of chi, clo,
    cn, rowmajor shaped as debug_prepared gives them -- None for a buffer the codebook never allocated.  The call leaves
    such a buffer unwritten: the arrays go in as 0xFF bytes, which no copy of finite rows comes back as."""
    d8, ng = (cb.dim + 7) // 8, (cb.n + 63) // 64
    raw = {"chi": np.full((ng, d8, 64, 8), 0xFFFF, np.uint16), "clo": np.full((ng, d8, 64, 8), 0xFFFF, np.uint16),
           "cn": np.full(ng * 64, 0xFFFFFFFF, np.uint32), "rowmajor": np.full((ng * 64, cb.dim), 0xFFFFFFFF, np.uint32)}
    flags = (C.c_int32 * 4)()
    u16, f32 = _lib.c_u16_p, _lib.c_float_p
    check(cb.e.lib.somhip_debug_prepared_state(cb.h, flags, _p(raw["chi"], u16), _p(raw["clo"], u16), _p(raw["cn"].view(np.float32), f32),
                                               _p(raw["rowmajor"].view(np.float32), f32)))
    out = {"prep_valid": flags[0], "rowmajor_valid": flags[1], "bm_open": flags[2], "bm_moved": flags[3]}
    for name, a in raw.items():
        untouched = (a.view(np.uint8) == 0xFF).all()
        out[name] = None if untouched else (a if a.dtype == np.uint16 else a.view(np.float32))
    return out


def debug_rerank_pairs(cb, ds, first, count, from_lists, pairs_cap=None):
    """The nearest-row search of data rows [first, first + count) with the re-rank's pairs selected from level 2's lists
    (from_lists) or from the whole matrix of group minima (somhip_debug_rerank_pairs): a dict of what the selection read
    (wmin, wmask [ngroups, bpad], gmin [bpad], tau [count]), what it wrote (colcount [4, ncols], overflow, pairs [n, 2] as
    (sample, row)) and the search's keys [count]."""
    ng, bp = (cb.n + 63) // 64, (count + 31) // 32 * 32
    ncols = bp // 32
    pairs_cap = pairs_cap if pairs_cap is not None else min(ncols * 16384, max(1 << 20, 64 * count))
    out = {"wmin": np.zeros((ng, bp), np.float32), "wmask": np.zeros((ng, bp), np.uint64), "gmin": np.zeros(bp, np.uint32),
           "tau": np.zeros(count, np.float32), "colcount": np.zeros((4, ncols), np.uint32),
           "keys": np.zeros(count, np.uint64)}
    pairs = np.zeros((pairs_cap, 2), np.uint32)
    overflow, npairs, bpad = np.zeros(1, np.uint32), C.c_int64(0), C.c_int64(0)
    check(cb.e.lib.somhip_debug_rerank_pairs(cb.h, ds.h, first, count, int(bool(from_lists)), _p(out["wmin"], _lib.c_float_p),
                                             _p(out["wmask"], _lib.c_u64_p), _p(out["gmin"], _lib.c_u32_p),
                                             _p(out["tau"], _lib.c_float_p), _p(out["colcount"], _lib.c_u32_p),
                                             _p(overflow, _lib.c_u32_p), _p(pairs, _lib.c_u32_p), pairs_cap, C.byref(npairs),
                                             _p(out["keys"], _lib.c_u64_p), C.byref(bpad)))
    assert bpad.value == bp
    out["overflow"] = int(overflow[0])
    out["pairs"] = pairs[:npairs.value].copy()
    return out


UPDATE_APPLY = ("gemm", "gauss_h", "gauss_s", "bubble_s", "run")
UPDATE_ENTRY = ("sample", "float4", "byte")


def update_plan(cb, ds, length, alpha, radius, count, alpha_type=ALPHA_LINEAR, use_fixed=0, use_weights=0, start_iter=0,
                data_first=None):
    """The plan of the mini-batch update of iterations [start_iter, start_iter + count) of a schedule of `length` on data
    rows from data_first (somhip_debug_update_plan; host arithmetic, no GPU work): a dict of the apply kernel and the
    stage choices before it, with the engine's current update mode."""
    data_first = start_iter % ds.n if data_first is None else data_first
    p = SomParams(length, alpha, radius, alpha_type, use_fixed, use_weights, count, start_iter, count, data_first)
    out = (C.c_int32 * 16)()
    check(cb.e.lib.somhip_debug_update_plan(cb.h, ds.h, C.byref(p), start_iter, count, data_first, out))
    return {"apply": UPDATE_APPLY[out[0]], "qw": out[1], "off32": bool(out[2]), "ntw": out[3], "decode": bool(out[4]),
            "members_nt": out[5], "members_rr": out[6], "entry": UPDATE_ENTRY[out[7]], "gauss_gemm": bool(out[8]),
            "tail": bool(out[9]), "tail_need": out[10], "reach_max": out[11], "order": bool(out[12]),
            "grid": out[13], "block": out[14]}


def som_train(cb, ds, length, alpha, radius, alpha_type=ALPHA_LINEAR, use_fixed=0, use_weights=0,
              batch=1, start_iter=0, count=None, data_first=None, trace=True):
    """som_training (reference som_rout.c:556); returns (trace_index, trace_diff)."""
    count = length - start_iter if count is None else count
    data_first = start_iter % ds.n if data_first is None else data_first
    p = SomParams(length, alpha, radius, alpha_type, use_fixed, use_weights, batch, start_iter, count,
                  data_first)
    ti = np.empty(count, dtype=np.int32) if trace else None
    td = np.empty(count, dtype=np.float32) if trace else None
    check(cb.e.lib.somhip_som_train(cb.h, ds.h, C.byref(p), _p(ti, _lib.c_i32_p), _p(td, _lib.c_float_p)))
    return ti, td


def batchmap_radius(radius, epochs, t):
    """r_t of epoch t of a batch-map run of `epochs` epochs from `radius`: the float the engine forms"""
    f = np.float32
    return f(f(1.0) + f(f(f(radius) - f(1.0)) * f(epochs - t)) / f(epochs))


def som_batchmap(cb, ds, epochs, radius, start_epoch=0, count=None, first=0, n=None, qerror=True):
    """Epochs [start_epoch, start_epoch + count) of Kohonen's batch map over data rows (first + s) % ds.n, s < n
    (somhip_som_batchmap): every epoch replaces each model vector by the neighbourhood-weighted mean of the data at the
    radius batchmap_radius(radius, epochs, t).  Returns float32[count], per epoch the quantization error (find_qerror's
    float sum) of the codebook the epoch started from, or None with qerror=False (no per-sample copy leaves the device)."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    p = _lib.BatchmapParams(epochs, radius, start_epoch, count, first, n)
    q = np.zeros(max(count, 0), dtype=np.float32) if qerror else None
    check(cb.e.lib.somhip_som_batchmap(cb.h, ds.h, C.byref(p), _p(q, _lib.c_float_p)))
    return q


def batchmap_sums(cb, ds, first=0, n=None):
    """The first stage of a batch-map epoch alone (somhip_debug_batchmap_sums): (hits uint32[cb.n], sums float64[cb.n, dim])
    -- per unit the samples it wins and the sum of their rows, one chain of fp64 additions in data order"""
    n = ds.n if n is None else n
    hits = np.zeros(cb.n, dtype=np.uint32)
    sums = np.zeros((cb.n, cb.dim), dtype=np.float64)
    check(cb.e.lib.somhip_debug_batchmap_sums(cb.h, ds.h, first, n, _p(hits, _lib.c_u32_p), _p(sums, _lib.c_double_p)))
    return hits, sums


def batchmap_combine(cb, r, hits, sums):
    """The second stage alone (somhip_debug_batchmap_combine): the codebook's rows become the neighbourhood-weighted means
    of `sums` over `hits` at radius r; a row whose neighbourhood holds no sample keeps its bits"""
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    assert hits.shape == (cb.n,) and sums.shape == (cb.n, cb.dim)
    check(cb.e.lib.somhip_debug_batchmap_combine(cb.h, float(np.float32(r)), _p(hits, _lib.c_u32_p), _p(sums, _lib.c_double_p)))


def batchmap_begin(cb):
    """Opens, or re-zeroes, the codebook's continued accumulation of a batch-map epoch (somhip_batchmap_begin): the data
    may then come in pieces, in order, and leave the bits of one som_batchmap epoch over the pieces' rows concatenated"""
    check(cb.e.lib.somhip_batchmap_begin(cb.h))


def batchmap_accumulate(cb, ds, first=0, n=None, qerror=True):
    """One piece (somhip_batchmap_accumulate): rows (first + s) % ds.n, s < n, of ds continue the per-unit fp64 chains, the
    counts and -- with qerror -- find_qerror's float chain"""
    n = ds.n if n is None else n
    check(cb.e.lib.somhip_batchmap_accumulate(cb.h, ds.h, first, n, 1 if qerror else 0))


def batchmap_finish(cb, r, group_first=0, group_count=None, qerror=True):
    """The combine at radius r from the accumulated state, for the destination row groups [group_first, + group_count) of
    (cb.n + 63) // 64 (somhip_batchmap_finish; all of them by default).  Returns the q chain as a float, or None."""
    group_count = (cb.n + 63) // 64 - group_first if group_count is None else group_count
    q = np.zeros(1, dtype=np.float32) if qerror else None
    check(cb.e.lib.somhip_batchmap_finish(cb.h, float(np.float32(r)), group_first, group_count, _p(q, _lib.c_float_p)))
    return float(q[0]) if qerror else None


def batchmap_end(cb):
    """Frees the accumulation's state (somhip_batchmap_end)"""
    check(cb.e.lib.somhip_batchmap_end(cb.h))


def batchmap_state(cb):
    """(device address, bytes) of the one blob that is the whole state (somhip_batchmap_state): [S | counts] as
    float64[cb.n, dim + 1], then 16 bytes {float32 q, uint32 unused, uint64 samples}"""
    addr, nbytes = C.c_void_p(), C.c_int64(0)
    check(cb.e.lib.somhip_batchmap_state(cb.h, C.byref(addr), C.byref(nbytes)))
    return int(addr.value), int(nbytes.value)


def som_batchmap_missing(cb, ds, epochs, radius, start_epoch=0, count=None, first=0, n=None, qerror=True):
    """som_batchmap over data with missing values (somhip_som_batchmap_missing): a sample is matched over the components
    it has, and a component of a model vector becomes the weighted mean of the samples that know it; a component no sample
    of the neighbourhood knows keeps its bits.  Arguments and return value are som_batchmap's; on data without masks the
    bits are som_batchmap's too."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    p = _lib.BatchmapParams(epochs, radius, start_epoch, count, first, n)
    q = np.zeros(max(count, 0), dtype=np.float32) if qerror else None
    check(cb.e.lib.somhip_som_batchmap_missing(cb.h, ds.h, C.byref(p), _p(q, _lib.c_float_p)))
    return q


def batchmap_missing_sums(cb, ds, first=0, n=None):
    """The first stage of such an epoch alone (somhip_debug_batchmap_missing_sums): (sums float64[cb.n, dim], counts
    float64[cb.n, dim]) -- per unit and component the fp64 chain over the samples the unit wins that know the component, in
    data order, and their number"""
    n = ds.n if n is None else n
    sums = np.zeros((cb.n, cb.dim), dtype=np.float64)
    counts = np.zeros((cb.n, cb.dim), dtype=np.float64)
    check(cb.e.lib.somhip_debug_batchmap_missing_sums(cb.h, ds.h, first, n, _p(sums, _lib.c_double_p), _p(counts, _lib.c_double_p)))
    return sums, counts


def batchmap_missing_combine(cb, r, sums, counts):
    """The second stage alone (somhip_debug_batchmap_missing_combine): every component of the codebook's rows becomes the
    neighbourhood-weighted mean of `sums` over `counts` at radius r; a component whose weighted count is 0 keeps its bits"""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.float64)
    assert sums.shape == (cb.n, cb.dim) and counts.shape == (cb.n, cb.dim)
    check(cb.e.lib.somhip_debug_batchmap_missing_combine(cb.h, float(np.float32(r)), _p(sums, _lib.c_double_p), _p(counts, _lib.c_double_p)))


def batchmap_missing_begin(cb):
    """batchmap_begin for data with missing values (somhip_batchmap_missing_begin): opens, or re-zeroes, a state of the form
    [S | C]; a codebook holds one batch-map accumulation, so an open one of the plain form is given up"""
    check(cb.e.lib.somhip_batchmap_missing_begin(cb.h))


def batchmap_missing_accumulate(cb, ds, first=0, n=None, qerror=True):
    """One piece (somhip_batchmap_missing_accumulate): as batchmap_accumulate, the piece may carry masks"""
    n = ds.n if n is None else n
    check(cb.e.lib.somhip_batchmap_missing_accumulate(cb.h, ds.h, first, n, 1 if qerror else 0))


def batchmap_missing_finish(cb, r, group_first=0, group_count=None, qerror=True):
    """The per-component combine at radius r from the accumulated state (somhip_batchmap_missing_finish); arguments and
    return value are batchmap_finish's"""
    group_count = (cb.n + 63) // 64 - group_first if group_count is None else group_count
    q = np.zeros(1, dtype=np.float32) if qerror else None
    check(cb.e.lib.somhip_batchmap_missing_finish(cb.h, float(np.float32(r)), group_first, group_count, _p(q, _lib.c_float_p)))
    return float(q[0]) if qerror else None


def batchmap_missing_end(cb):
    """Frees the accumulation's state (somhip_batchmap_missing_end)"""
    check(cb.e.lib.somhip_batchmap_missing_end(cb.h))


def batchmap_missing_state(cb):
    """(device address, bytes) of the state (somhip_batchmap_missing_state): [S | C] as float64[cb.n, 2 * dim], a row
    holding a unit's dim sums and behind them its dim counts, then 16 bytes {float32 q, uint32 unused, uint64 samples}"""
    addr, nbytes = C.c_void_p(), C.c_int64(0)
    check(cb.e.lib.somhip_batchmap_missing_state(cb.h, C.byref(addr), C.byref(nbytes)))
    return int(addr.value), int(nbytes.value)


GLVQ_PLAN, GLVQ_DIRECT, GLVQ_LIST = -1, 0, 1


def glvq_alpha(alpha, epochs, t):
    """alpha_t of epoch t of a GLVQ run of `epochs` epochs from `alpha`: the float the engine forms"""
    f = np.float32
    return f(f(f(alpha) * f(epochs - t)) / f(epochs))


def glvq_plan(n_rows, dim, n, lib=None):
    """The route glvq_train's search takes for this shape (somhip_debug_glvq_plan): GLVQ_DIRECT or GLVQ_LIST.  Host
    arithmetic: no GPU needed."""
    lib = lib or _lib.load()
    route = C.c_int32(0)
    check(lib.somhip_debug_glvq_plan(n_rows, dim, n, C.byref(route)))
    return route.value


def glvq_train(cb, ds, epochs, alpha, sigmoid_beta=0.0, start_epoch=0, count=None, first=0, n=None, stats=True):
    """Epochs [start_epoch, start_epoch + count) of batch GLVQ over data rows (first + s) % ds.n, s < n (somhip_glvq_train):
    every epoch is one full-batch gradient step of E = mean f(mu) at the rate glvq_alpha(alpha, epochs, t).  alpha has the
    unit of a squared distance.  Returns (cost float64[count], correct int64[count]) of the codebook each epoch started
    from, or None with stats=False."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    p = _lib.GlvqParams(epochs, start_epoch, count, first, n, alpha, sigmoid_beta)
    cost = np.zeros(max(count, 0), dtype=np.float64) if stats else None
    correct = np.zeros(max(count, 0), dtype=np.int64) if stats else None
    check(cb.e.lib.somhip_glvq_train(cb.h, ds.h, C.byref(p), _p(cost, _lib.c_double_p), _p(correct, _lib.c_i64_p)))
    return (cost, correct) if stats else None


def glvq_search(cb, ds, first=0, n=None, route=GLVQ_PLAN):
    """The class-wise winner search alone (somhip_debug_glvq_search): (dplus float32[n], iplus int32[n], dminus, iminus,
    remainder) -- per sample the nearest row of its own class and of any other, and how many samples went through the
    class-wise scan (all of them on the direct route)"""
    n = ds.n if n is None else n
    dp, dm = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    ip, im = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rem = C.c_int64(0)
    check(cb.e.lib.somhip_debug_glvq_search(cb.h, ds.h, first, n, route, _p(dp, _lib.c_float_p), _p(ip, _lib.c_i32_p),
                                            _p(dm, _lib.c_float_p), _p(im, _lib.c_i32_p), C.byref(rem)))
    return dp, ip, dm, im, rem.value


def glvq_sums(cb, ds, first=0, n=None, sigmoid_beta=0.0):
    """Search, terms and sums of a GLVQ epoch (somhip_debug_glvq_sums), as a dict: xi_plus, xi_minus, f float64[n];
    sums_plus, sums_minus float64[cb.n, dim + 1] (the last column is the sum of xi); n_plus, n_minus uint32[cb.n];
    cost float64[cb.n]; correct"""
    n = ds.n if n is None else n
    d = lambda *shape: np.zeros(shape, dtype=np.float64)
    out = {"xi_plus": d(n), "xi_minus": d(n), "f": d(n), "sums_plus": d(cb.n, cb.dim + 1), "sums_minus": d(cb.n, cb.dim + 1),
           "n_plus": np.zeros(cb.n, dtype=np.uint32), "n_minus": np.zeros(cb.n, dtype=np.uint32), "cost": d(cb.n)}
    correct = C.c_int64(0)
    dp, up = _lib.c_double_p, _lib.c_u32_p
    check(cb.e.lib.somhip_debug_glvq_sums(cb.h, ds.h, first, n, sigmoid_beta, _p(out["xi_plus"], dp), _p(out["xi_minus"], dp),
                                          _p(out["f"], dp), _p(out["sums_plus"], dp), _p(out["n_plus"], up),
                                          _p(out["sums_minus"], dp), _p(out["n_minus"], up), _p(out["cost"], dp), C.byref(correct)))
    out["correct"] = correct.value
    return out


def glvq_update(cb, alpha_t, n, sums_plus, n_plus, sums_minus, n_minus):
    """The update alone (somhip_debug_glvq_update) from host-supplied sums as glvq_sums returns them, with
    a = float64(alpha_t) / n; a row with n_plus == n_minus == 0 keeps its bits"""
    sp, sm = np.ascontiguousarray(sums_plus, dtype=np.float64), np.ascontiguousarray(sums_minus, dtype=np.float64)
    cp, cm = np.ascontiguousarray(n_plus, dtype=np.uint32), np.ascontiguousarray(n_minus, dtype=np.uint32)
    assert sp.shape == sm.shape == (cb.n, cb.dim + 1) and cp.shape == cm.shape == (cb.n,)
    check(cb.e.lib.somhip_debug_glvq_update(cb.h, float(np.float32(alpha_t)), n, _p(sp, _lib.c_double_p), _p(cp, _lib.c_u32_p),
                                            _p(sm, _lib.c_double_p), _p(cm, _lib.c_u32_p)))


def glvq_begin(cb):
    """Opens, or re-zeroes, the codebook's continued accumulation of a GLVQ epoch (somhip_glvq_begin): the data may then
    come in pieces, in order, and leave the bits of one glvq_train epoch over the pieces' rows concatenated"""
    check(cb.e.lib.somhip_glvq_begin(cb.h))


def glvq_accumulate(cb, ds, first=0, n=None, sigmoid_beta=0.0):
    """One piece (somhip_glvq_accumulate): search, terms and grouping of rows (first + s) % ds.n, s < n, of ds against the
    codebook as it stands; the per-row fp64 chains, the counts and the tail go on from the state"""
    n = ds.n if n is None else n
    check(cb.e.lib.somhip_glvq_accumulate(cb.h, ds.h, first, n, sigmoid_beta))


def glvq_finish(cb, alpha_t):
    """The update from the state with a = float64(alpha_t) / samples (somhip_glvq_finish).  Returns (cost, correct,
    samples): what one glvq_train epoch reports, and the samples the pieces held."""
    cost, correct, samples = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
    check(cb.e.lib.somhip_glvq_finish(cb.h, float(np.float32(alpha_t)), C.byref(cost), C.byref(correct), C.byref(samples)))
    return cost.value, correct.value, samples.value


def glvq_end(cb):
    """Frees the accumulation's state (somhip_glvq_end)"""
    check(cb.e.lib.somhip_glvq_end(cb.h))


def glvq_state(cb):
    """(device address, bytes) of the one blob that is the whole state (somhip_glvq_state): [Sp | sp] and [Sm | sm] as
    float64[2, cb.n, dim + 1], cost float64[cb.n], np and nm uint32[cb.n] each, then 16 bytes {uint64 samples, uint64
    correct}"""
    addr, nbytes = C.c_void_p(), C.c_int64(0)
    check(cb.e.lib.somhip_glvq_state(cb.h, C.byref(addr), C.byref(nbytes)))
    return int(addr.value), int(nbytes.value)


def glvq_state_arrays(cb):
    """The state blob on the host, taken apart as glvq_sums names its parts: a dict of sums_plus, sums_minus
    float64[cb.n, dim + 1], cost float64[cb.n], n_plus, n_minus uint32[cb.n], samples, correct"""
    addr, nbytes = glvq_state(cb)
    blob = cb.e.copy_to_host(addr, nbytes)
    ld, r = cb.dim + 1, cb.n
    s_bytes, c_bytes = 8 * 2 * r * ld, 8 * r
    assert nbytes == s_bytes + c_bytes + 8 * r + 16
    S = blob[:s_bytes].view(np.float64).reshape(2, r, ld)
    counts = blob[s_bytes + c_bytes:s_bytes + c_bytes + 8 * r].view(np.uint32).reshape(2, r)
    tail = blob[s_bytes + c_bytes + 8 * r:].view(np.uint64)
    return {"sums_plus": S[0].copy(), "sums_minus": S[1].copy(), "cost": blob[s_bytes:s_bytes + c_bytes].view(np.float64).copy(),
            "n_plus": counts[0].copy(), "n_minus": counts[1].copy(), "samples": int(tail[0]), "correct": int(tail[1])}


def glvq_train_ranks(cb, block, comm, epochs, alpha, sigmoid_beta=0.0, start_epoch=0, count=None, first=0, n=None, stats=True):
    """glvq_train over the row blocks of the ranks of `comm` (a somhip_comm handle), this rank's block being rows
    (first + s) % block.n, s < n, of `block` (somhip_glvq_train_ranks; block None with n 0: a rank without rows).  Every
    rank ends with the rows of glvq_train over the blocks in rank order.  Returns (cost, correct) or None."""
    count = epochs - start_epoch if count is None else count
    n = (block.n if block is not None else 0) if n is None else n
    p = _lib.GlvqParams(epochs, start_epoch, count, first, n, alpha, sigmoid_beta)
    cost = np.zeros(max(count, 0), dtype=np.float64) if stats else None
    correct = np.zeros(max(count, 0), dtype=np.int64) if stats else None
    check(cb.e.lib.somhip_glvq_train_ranks(cb.h, block.h if block is not None else None, C.byref(p), comm,
                                           _p(cost, _lib.c_double_p), _p(correct, _lib.c_i64_p)))
    return (cost, correct) if stats else None


def _ng_params(units, epochs, lambda0, lambda_end, ranks, start_epoch=0, count=0, first=0, n=0):
    lambda0 = min(units, 256) / 2.0 if lambda0 is None else lambda0
    return _lib.NgParams(epochs, lambda0, lambda_end, ranks, start_epoch, count, first, n)


def ng_schedule(units, epochs, t, lambda0=None, lambda_end=0.01, ranks=0, lib=None):
    """Epoch t of a neural-gas run of `epochs` epochs on `units` rows (somhip_debug_ng_schedule): (lambda_t float,
    K_t int, w float64[K_t]) exactly as the engine forms them -- lambda0 None is min(units, 256) / 2.  Host arithmetic:
    no GPU needed."""
    lib = lib or _lib.load()
    p = _ng_params(units, epochs, lambda0, lambda_end, ranks)
    lam, k = C.c_double(0), C.c_int32(0)
    w = np.zeros(256, dtype=np.float64)
    check(lib.somhip_debug_ng_schedule(C.byref(p), units, t, C.byref(lam), C.byref(k), _p(w, _lib.c_double_p)))
    return lam.value, k.value, w[:k.value].copy()


def ng_train(cb, ds, epochs, lambda0=None, lambda_end=0.01, ranks=0, start_epoch=0, count=None, first=0, n=None, qerror=True):
    """Epochs [start_epoch, start_epoch + count) of batch neural gas over data rows (first + s) % ds.n, s < n
    (somhip_ng_train): every epoch replaces each row by the mean of the data weighted by exp(-rank / lambda_t), over the
    first K_t ranks of every sample (ng_schedule).  Beyond 256 rows the ranks are truncated at the 256 nearest.  Returns
    float32[count], per epoch the quantization error (find_qerror's float sum) of the codebook the epoch started from, or
    None with qerror=False (no per-sample copy leaves the device)."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    p = _ng_params(cb.n, epochs, lambda0, lambda_end, ranks, start_epoch, count, first, n)
    q = np.zeros(max(count, 0), dtype=np.float32) if qerror else None
    check(cb.e.lib.somhip_ng_train(cb.h, ds.h, C.byref(p), _p(q, _lib.c_float_p)))
    return q


def ng_ranks(cb, ds, K, first=0, n=None):
    """The rank search alone (somhip_debug_ng_ranks): (units int32[n, K], dist float32[n, K]) -- per sample its K nearest
    rows, nearest first, the later row first among equal distances; -1 / -1.0 where the codebook has no such row"""
    n = ds.n if n is None else n
    units = np.zeros((n, K), dtype=np.int32)
    dist = np.zeros((n, K), dtype=np.float32)
    check(cb.e.lib.somhip_debug_ng_ranks(cb.h, ds.h, first, n, K, _p(units, _lib.c_i32_p), _p(dist, _lib.c_float_p)))
    return units, dist


def ng_sums(cb, ds, weights, first=0, n=None, segment=0):
    """Ranks, grouping and sums of a neural-gas epoch with K = len(weights) ranks (somhip_debug_ng_sums): (hits uint32[cb.n],
    sums float64[cb.n, dim], wsum float64[cb.n]) -- per unit the samples that rank it, and one chain of fp64 additions in
    data order of w[rank] * x and of w[rank].  segment: samples per segment (0: the engine's rule); same bits for all."""
    n = ds.n if n is None else n
    w = np.ascontiguousarray(weights, dtype=np.float64)
    hits = np.zeros(cb.n, dtype=np.uint32)
    sums = np.zeros((cb.n, cb.dim), dtype=np.float64)
    wsum = np.zeros(cb.n, dtype=np.float64)
    check(cb.e.lib.somhip_debug_ng_sums(cb.h, ds.h, first, n, len(w), _p(w, _lib.c_double_p), segment, _p(hits, _lib.c_u32_p),
                                        _p(sums, _lib.c_double_p), _p(wsum, _lib.c_double_p)))
    return hits, sums, wsum


def ng_update(cb, hits, sums, wsum):
    """The update alone (somhip_debug_ng_update) from host-supplied sums as ng_sums returns them: row j becomes
    float32(sums[j] / wsum[j]) where wsum[j] > 0 and keeps its bits elsewhere"""
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    wsum = np.ascontiguousarray(wsum, dtype=np.float64)
    assert hits.shape == wsum.shape == (cb.n,) and sums.shape == (cb.n, cb.dim)
    check(cb.e.lib.somhip_debug_ng_update(cb.h, _p(hits, _lib.c_u32_p), _p(sums, _lib.c_double_p), _p(wsum, _lib.c_double_p)))


NG_DENSE_MAX = 4096      # SOMHIP_NG_DENSE_MAX: the most rows of a codebook the dense form takes


def ng_dense_schedule(units, epochs, t, lambda0=None, lambda_end=0.01, lib=None):
    """Epoch t of a dense neural-gas run of `epochs` epochs on `units` rows (somhip_debug_ng_dense_schedule): (lambda_t
    float, w float64[units]) exactly as the engine forms them: ng_schedule's lambda_t and exp(-r / lambda_t) for every
    rank, +0.0 where it underflows.  Host arithmetic: no GPU needed."""
    lib = lib or _lib.load()
    p = _ng_params(units, epochs, lambda0, lambda_end, 0)
    lam = C.c_double(0)
    w = np.zeros(units, dtype=np.float64)
    check(lib.somhip_debug_ng_dense_schedule(C.byref(p), units, t, C.byref(lam), _p(w, _lib.c_double_p)))
    return lam.value, w


def ng_train_dense(cb, ds, epochs, lambda0=None, lambda_end=0.01, ranks=0, start_epoch=0, count=None, first=0, n=None, qerror=True):
    """Epochs [start_epoch, start_epoch + count) of dense batch neural gas over data rows (first + s) % ds.n, s < n
    (somhip_ng_train_dense): every epoch replaces each row by the mean of the data weighted by exp(-rank / lambda_t), the
    rank taken among ALL rows (at most NG_DENSE_MAX of them) -- ng_train without its truncation at 256 ranks, the sums
    formed on the fp64 MFMA.  ranks must be 0.  Returns float32[count], per epoch the quantization error (find_qerror's
    float sum) of the codebook the epoch started from, or None with qerror=False."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    p = _ng_params(cb.n, epochs, lambda0, lambda_end, ranks, start_epoch, count, first, n)
    q = np.zeros(max(count, 0), dtype=np.float32) if qerror else None
    check(cb.e.lib.somhip_ng_train_dense(cb.h, ds.h, C.byref(p), _p(q, _lib.c_float_p)))
    return q


def ng_dense_ranks(cb, ds, first=0, n=None):
    """The full ranking alone (somhip_debug_ng_dense_ranks): (rank int32[n, cb.n], dist float32[n, cb.n]) -- per sample
    and unit the number of units before it in the order (distance ascending, the later row first among equal distances),
    and its squared distance"""
    n = ds.n if n is None else n
    rank = np.zeros((max(n, 0), cb.n), dtype=np.int32)
    dist = np.zeros((max(n, 0), cb.n), dtype=np.float32)
    check(cb.e.lib.somhip_debug_ng_dense_ranks(cb.h, ds.h, first, n, _p(rank, _lib.c_i32_p), _p(dist, _lib.c_float_p)))
    return rank, dist


def ng_dense_sums(cb, ds, lam, first=0, n=None, chunk=0):
    """Distances, ranking and sums of a dense neural-gas epoch at lambda = lam (somhip_debug_ng_dense_sums): (sums
    float64[cb.n, dim], wsum float64[cb.n]) = Q^T [X | 1] with Q[s][j] = exp(-rank[s][j] / lam).  chunk: samples per cut, a
    multiple of 64 (0: the engine's own); same bits for all.  ng_update takes the pair (its hits are not read)."""
    n = ds.n if n is None else n
    sums = np.zeros((cb.n, cb.dim), dtype=np.float64)
    wsum = np.zeros(cb.n, dtype=np.float64)
    check(cb.e.lib.somhip_debug_ng_dense_sums(cb.h, ds.h, first, n, lam, chunk, _p(sums, _lib.c_double_p), _p(wsum, _lib.c_double_p)))
    return sums, wsum


def _grlvq_lambda(cb, lam):
    """a float32[dim] copy of the relevance vector the call may write; None: 1 / dim each"""
    if lam is None:
        return np.full(cb.dim, np.float32(1.0) / np.float32(cb.dim), dtype=np.float32)
    lam = np.array(lam, dtype=np.float32).reshape(-1)
    if lam.shape != (cb.dim,):
        raise ValueError("lambda has %d entries, the codebook %d components" % (lam.size, cb.dim))
    return lam


def grlvq_train(cb, ds, epochs, alpha, eps, lam=None, sigmoid_beta=0.0, start_epoch=0, count=None, first=0, n=None, stats=True):
    """Epochs [start_epoch, start_epoch + count) of batch GRLVQ over data rows (first + s) % ds.n, s < n
    (somhip_grlvq_train): batch GLVQ under d_lambda = sum_k lambda[k] (x[k] - w[k])^2, the relevances lambda learned at the
    rate glvq_alpha(eps, epochs, t) by the gradient that moves the rows, clamped at 0 and normalised to sum 1 after every
    step.  lam: the relevances the call starts from, taken as they are (None: 1 / dim each); eps = 0 leaves them alone.
    Returns (lambda float32[dim], cost float64[count], correct int64[count]) -- cost and correct of the state each epoch
    started from -- or lambda alone with stats=False.  Hand lambda on to continue a run."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    lam = _grlvq_lambda(cb, lam)
    p = _lib.GrlvqParams(epochs, start_epoch, count, first, n, alpha, sigmoid_beta, eps)
    cost = np.zeros(max(count, 0), dtype=np.float64) if stats else None
    correct = np.zeros(max(count, 0), dtype=np.int64) if stats else None
    check(cb.e.lib.somhip_grlvq_train(cb.h, ds.h, C.byref(p), _p(lam, _lib.c_float_p), _p(cost, _lib.c_double_p),
                                      _p(correct, _lib.c_i64_p)))
    return (lam, cost, correct) if stats else lam


def grlvq_search(cb, ds, lam=None, first=0, n=None):
    """The class-wise winner search under d_lambda (somhip_grlvq_search): (dplus float32[n], iplus int32[n], dminus,
    iminus) -- per sample the nearest row of its own class and of any other.  A sample is classified correctly where
    (dplus, iplus) < (dminus, iminus)."""
    n = ds.n if n is None else n
    lam = _grlvq_lambda(cb, lam)
    dp, dm = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    ip, im = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    check(cb.e.lib.somhip_grlvq_search(cb.h, ds.h, first, n, _p(lam, _lib.c_float_p), _p(dp, _lib.c_float_p), _p(ip, _lib.c_i32_p),
                                       _p(dm, _lib.c_float_p), _p(im, _lib.c_i32_p)))
    return dp, ip, dm, im


def grlvq_sums(cb, ds, lam=None, first=0, n=None, sigmoid_beta=0.0):
    """Search, terms, sums and relevance gradient of a GRLVQ epoch (somhip_debug_grlvq_sums), as a dict: glvq_sums' entries
    under d_lambda, and rel_plus, rel_minus float64[cb.n, dim] (Rp, Rm), grad float64[dim] (G)"""
    n = ds.n if n is None else n
    lam = _grlvq_lambda(cb, lam)
    d = lambda *shape: np.zeros(shape, dtype=np.float64)
    out = {"xi_plus": d(n), "xi_minus": d(n), "f": d(n), "sums_plus": d(cb.n, cb.dim + 1), "sums_minus": d(cb.n, cb.dim + 1),
           "n_plus": np.zeros(cb.n, dtype=np.uint32), "n_minus": np.zeros(cb.n, dtype=np.uint32), "cost": d(cb.n),
           "rel_plus": d(cb.n, cb.dim), "rel_minus": d(cb.n, cb.dim), "grad": d(cb.dim)}
    correct = C.c_int64(0)
    dp, up = _lib.c_double_p, _lib.c_u32_p
    check(cb.e.lib.somhip_debug_grlvq_sums(cb.h, ds.h, first, n, sigmoid_beta, _p(lam, _lib.c_float_p), _p(out["xi_plus"], dp),
                                           _p(out["xi_minus"], dp), _p(out["f"], dp), _p(out["sums_plus"], dp), _p(out["n_plus"], up),
                                           _p(out["sums_minus"], dp), _p(out["n_minus"], up), _p(out["cost"], dp), C.byref(correct),
                                           _p(out["rel_plus"], dp), _p(out["rel_minus"], dp), _p(out["grad"], dp)))
    out["correct"] = correct.value
    return out


def grlvq_update(cb, alpha_t, eps_t, n, lam, sums_plus, n_plus, sums_minus, n_minus, grad):
    """The update and the relevance step alone (somhip_debug_grlvq_update) from host-supplied sums as grlvq_sums returns
    them: the rows move with a = float64(alpha_t) / n and the lambda given; returns the lambda after the step with eps_t
    (the bits of the one given where eps_t == 0 or every component is clamped)"""
    sp, sm = np.ascontiguousarray(sums_plus, dtype=np.float64), np.ascontiguousarray(sums_minus, dtype=np.float64)
    cp, cm = np.ascontiguousarray(n_plus, dtype=np.uint32), np.ascontiguousarray(n_minus, dtype=np.uint32)
    g = np.ascontiguousarray(grad, dtype=np.float64)
    assert sp.shape == sm.shape == (cb.n, cb.dim + 1) and cp.shape == cm.shape == (cb.n,) and g.shape == (cb.dim,)
    lam = _grlvq_lambda(cb, lam)
    check(cb.e.lib.somhip_debug_grlvq_update(cb.h, float(np.float32(alpha_t)), float(np.float32(eps_t)), n, _p(lam, _lib.c_float_p),
                                             _p(sp, _lib.c_double_p), _p(cp, _lib.c_u32_p), _p(sm, _lib.c_double_p),
                                             _p(cm, _lib.c_u32_p), _p(g, _lib.c_double_p)))
    return lam


def gmlvq_omega(dim, rank=None):
    """the matrix a GMLVQ run starts from where none is given: float32[rank, dim] with (float)(1 / sqrt(dim)) where
    k % rank == r and 0 elsewhere -- every component takes part, trace(Omega^T Omega) is 1"""
    rank = dim if rank is None else rank
    om = np.zeros((rank, dim), dtype=np.float32)
    k = np.arange(dim)
    om[k % rank, k] = np.float32(1.0 / np.sqrt(np.float64(dim)))
    return om


def _gmlvq_omega(cb, omega):
    """a float32[rank, dim] copy of the matrix the call may write; None: gmlvq_omega(dim)"""
    if omega is None:
        return gmlvq_omega(cb.dim)
    omega = np.array(omega, dtype=np.float32, ndmin=2)
    if omega.ndim != 2 or omega.shape[1] != cb.dim:
        raise ValueError("omega has shape %s, the codebook %d components" % (omega.shape, cb.dim))
    return np.ascontiguousarray(omega)


def gmlvq_train(cb, ds, epochs, alpha, eps, omega=None, sigmoid_beta=0.0, start_epoch=0, count=None, first=0, n=None, stats=True):
    """Epochs [start_epoch, start_epoch + count) of batch GMLVQ over data rows (first + s) % ds.n, s < n
    (somhip_gmlvq_train): batch GLVQ under d(x, w) = |Omega (x - w)|^2, the matrix Omega [rank, dim] learned at the rate
    glvq_alpha(eps, epochs, t) by the gradient that moves the rows and scaled to trace(Omega^T Omega) = 1 after every
    step.  omega: the matrix the call starts from, taken as it is (None: gmlvq_omega(dim)); its rows are the rank; eps = 0
    leaves it alone.  Returns (omega float32[rank, dim], cost float64[count], correct int64[count]) -- cost and correct of
    the state each epoch started from -- or omega alone with stats=False.  Hand omega on to continue a run."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    om = _gmlvq_omega(cb, omega)
    p = _lib.GmlvqParams(epochs, start_epoch, count, first, n, alpha, sigmoid_beta, eps, om.shape[0])
    cost = np.zeros(max(count, 0), dtype=np.float64) if stats else None
    correct = np.zeros(max(count, 0), dtype=np.int64) if stats else None
    check(cb.e.lib.somhip_gmlvq_train(cb.h, ds.h, C.byref(p), _p(om, _lib.c_float_p), _p(cost, _lib.c_double_p),
                                      _p(correct, _lib.c_i64_p)))
    return (om, cost, correct) if stats else om


def gmlvq_search(cb, ds, omega=None, first=0, n=None):
    """The class-wise winner search under |Omega (x - w)|^2 (somhip_gmlvq_search): (dplus float32[n], iplus int32[n],
    dminus, iminus) -- per sample the nearest row of its own class and of any other.  A sample is classified correctly
    where (dplus, iplus) < (dminus, iminus)."""
    n = ds.n if n is None else n
    om = _gmlvq_omega(cb, omega)
    dp, dm = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    ip, im = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    check(cb.e.lib.somhip_gmlvq_search(cb.h, ds.h, first, n, _p(om, _lib.c_float_p), om.shape[0], _p(dp, _lib.c_float_p),
                                       _p(ip, _lib.c_i32_p), _p(dm, _lib.c_float_p), _p(im, _lib.c_i32_p)))
    return dp, ip, dm, im


def gmlvq_project(cb, ds=None, omega=None, first=0, n=None):
    """Omega applied to rows (somhip_gmlvq_project): float32[n, rank] for data rows (first + s) % ds.n, s < n, or, with ds
    None, float32[cb.n, rank] for the codebook's rows -- the values the search reads, and the picture at rank 2"""
    om = _gmlvq_omega(cb, omega)
    n = (cb.n if ds is None else ds.n) if n is None else n
    out = np.zeros((max(n, 0), om.shape[0]), dtype=np.float32)
    check(cb.e.lib.somhip_gmlvq_project(cb.h, None if ds is None else ds.h, first, n, _p(om, _lib.c_float_p), om.shape[0],
                                        _p(out, _lib.c_float_p)))
    return out


def gmlvq_sums(cb, ds, omega=None, first=0, n=None, sigmoid_beta=0.0):
    """Projection, search, terms, sums and the gradient of omega of a GMLVQ epoch (somhip_debug_gmlvq_sums), as a dict:
    glvq_sums' entries under the projected distance, and grad float64[rank, dim] (Gm)"""
    n = ds.n if n is None else n
    om = _gmlvq_omega(cb, omega)
    d = lambda *shape: np.zeros(shape, dtype=np.float64)
    out = {"xi_plus": d(n), "xi_minus": d(n), "f": d(n), "sums_plus": d(cb.n, cb.dim + 1), "sums_minus": d(cb.n, cb.dim + 1),
           "n_plus": np.zeros(cb.n, dtype=np.uint32), "n_minus": np.zeros(cb.n, dtype=np.uint32), "cost": d(cb.n),
           "grad": d(om.shape[0], cb.dim)}
    correct = C.c_int64(0)
    dp, up = _lib.c_double_p, _lib.c_u32_p
    check(cb.e.lib.somhip_debug_gmlvq_sums(cb.h, ds.h, first, n, sigmoid_beta, _p(om, _lib.c_float_p), om.shape[0],
                                           _p(out["xi_plus"], dp), _p(out["xi_minus"], dp), _p(out["f"], dp), _p(out["sums_plus"], dp),
                                           _p(out["n_plus"], up), _p(out["sums_minus"], dp), _p(out["n_minus"], up), _p(out["cost"], dp),
                                           C.byref(correct), _p(out["grad"], dp)))
    out["correct"] = correct.value
    return out


def gmlvq_update(cb, alpha_t, eps_t, n, omega, sums_plus, n_plus, sums_minus, n_minus, grad):
    """The update and omega's step alone (somhip_debug_gmlvq_update) from host-supplied sums as gmlvq_sums returns them:
    the rows move with a = float64(alpha_t) / n through the omega given; returns the omega after the step with eps_t (the
    bits of the one given where eps_t == 0 or the step lands on the zero matrix)"""
    sp, sm = np.ascontiguousarray(sums_plus, dtype=np.float64), np.ascontiguousarray(sums_minus, dtype=np.float64)
    cp, cm = np.ascontiguousarray(n_plus, dtype=np.uint32), np.ascontiguousarray(n_minus, dtype=np.uint32)
    om = _gmlvq_omega(cb, omega)
    g = np.ascontiguousarray(grad, dtype=np.float64)
    assert sp.shape == sm.shape == (cb.n, cb.dim + 1) and cp.shape == cm.shape == (cb.n,) and g.shape == om.shape
    check(cb.e.lib.somhip_debug_gmlvq_update(cb.h, float(np.float32(alpha_t)), float(np.float32(eps_t)), n, _p(om, _lib.c_float_p),
                                             om.shape[0], _p(sp, _lib.c_double_p), _p(cp, _lib.c_u32_p), _p(sm, _lib.c_double_p),
                                             _p(cm, _lib.c_u32_p), _p(g, _lib.c_double_p)))
    return om


def rslvq_chunk(n_rows, lib=None):
    """(chunk, ld) of a codebook of n_rows rows (somhip_debug_rslvq_chunk): the samples per chunk that rslvq_train and
    rslvq_search take, and the leading dimension 64 * ceil(n_rows / 64) of the coefficients.  Host arithmetic: no GPU needed."""
    lib = lib or _lib.load()
    chunk, ld = C.c_int64(0), C.c_int64(0)
    check(lib.somhip_debug_rslvq_chunk(n_rows, C.byref(chunk), C.byref(ld)))
    return chunk.value, ld.value


def rslvq_train(cb, ds, epochs, alpha, sigma2, start_epoch=0, count=None, first=0, n=None, stats=True):
    """Epochs [start_epoch, start_epoch + count) of batch Robust Soft LVQ over data rows (first + s) % ds.n, s < n
    (somhip_rslvq_train): every epoch is one full-batch gradient step of E = mean -log P(y | x) under a Gaussian mixture
    of squared width sigma2 at the rate glvq_alpha(alpha, epochs, t) / sigma2.  alpha has the unit of a squared distance.
    Returns (cost float64[count], correct int64[count]) of the codebook each epoch started from, or None with stats=False."""
    count = epochs - start_epoch if count is None else count
    n = ds.n if n is None else n
    p = _lib.RslvqParams(epochs, start_epoch, count, first, n, alpha, sigma2)
    cost = np.zeros(max(count, 0), dtype=np.float64) if stats else None
    correct = np.zeros(max(count, 0), dtype=np.int64) if stats else None
    check(cb.e.lib.somhip_rslvq_train(cb.h, ds.h, C.byref(p), _p(cost, _lib.c_double_p), _p(correct, _lib.c_i64_p)))
    return (cost, correct) if stats else None


def rslvq_search(cb, ds, sigma2, first=0, n=None, pown=True):
    """The evaluation of a model (somhip_rslvq_search): (cost, correct, pown float64[n] or None) -- the mean of
    -log P(y | x), the samples whose nearest row carries their label, and P(y | x) per sample.  The rows are not touched."""
    n = ds.n if n is None else n
    cost, correct = C.c_double(0), C.c_int64(0)
    po = np.zeros(n, dtype=np.float64) if pown else None
    check(cb.e.lib.somhip_rslvq_search(cb.h, ds.h, first, n, sigma2, C.byref(cost), C.byref(correct), _p(po, _lib.c_double_p)))
    return cost.value, correct.value, po


def rslvq_posterior(cb, ds, sigma2, first=0, n=None, chunk=0):
    """Distances and posteriors of an RSLVQ epoch (somhip_debug_rslvq_posterior), as a dict: q float64[n, ld] (the
    coefficients, zeros behind column cb.n), cost float64[n], correct int32[n], pown float64[n].  chunk: the samples per
    launch, a multiple of 64 (0: rslvq_chunk's)."""
    n = ds.n if n is None else n
    ld = rslvq_chunk(cb.n, cb.e.lib)[1]
    out = {"q": np.full((n, ld), np.nan), "cost": np.zeros(n), "correct": np.zeros(n, dtype=np.int32), "pown": np.zeros(n)}
    dp = _lib.c_double_p
    check(cb.e.lib.somhip_debug_rslvq_posterior(cb.h, ds.h, first, n, sigma2, chunk, _p(out["q"], dp), _p(out["cost"], dp),
                                                _p(out["correct"], _lib.c_i32_p), _p(out["pown"], dp)))
    return out


def rslvq_sums(cb, ds, q, first=0, n=None, chunk=0):
    """[G | c] = Q^T [X | 1] alone (somhip_debug_rslvq_sums) on the caller's q float64[n, cb.n] or [n, ld]: (G float64[cb.n,
    dim], c float64[cb.n])"""
    n = ds.n if n is None else n
    ld = rslvq_chunk(cb.n, cb.e.lib)[1]
    q = np.asarray(q, dtype=np.float64)
    assert q.shape in ((n, cb.n), (n, ld)), q.shape
    qp = np.zeros((n, ld), dtype=np.float64)
    qp[:, :q.shape[1]] = q
    G, c = np.zeros((cb.n, cb.dim), dtype=np.float64), np.zeros(cb.n, dtype=np.float64)
    dp = _lib.c_double_p
    check(cb.e.lib.somhip_debug_rslvq_sums(cb.h, ds.h, first, n, chunk, _p(qp, dp), _p(G, dp), _p(c, dp)))
    return G, c


def rslvq_update(cb, alpha_t, sigma2, n, G, c):
    """The update alone (somhip_debug_rslvq_update) from host-supplied sums as rslvq_sums returns them, with
    a = float64(alpha_t) / (float64(sigma2) * n); every row is stepped"""
    G, c = np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    assert G.shape == (cb.n, cb.dim) and c.shape == (cb.n,)
    check(cb.e.lib.somhip_debug_rslvq_update(cb.h, float(np.float32(alpha_t)), float(np.float32(sigma2)), n, _p(G, _lib.c_double_p),
                                             _p(c, _lib.c_double_p)))


def _distortion_totals(tot):
    return {"energy": tot.energy, "scale": tot.scale, "samples": tot.samples}


class Distortion:
    """The state of a map distortion on the device (somhip_distortion), made for the shape of `cb`: per unit the samples
    it wins, the fp64 sums of their rows and of their squared norms.  accumulate adds data to it piece by piece -- any cut
    leaves the bits of one call; evaluate gives the energy E(r) = sum_s sum_j h_r(c(s), j) |x_s - m_j|^2 of the
    codebook's current rows under the accumulated winners.  It lives until closed."""

    def __init__(self, cb):
        self.e = cb.e
        self.n, self.dim = cb.n, cb.dim
        h = C.c_void_p()
        check(cb.e.lib.somhip_distortion_create(cb.h, C.byref(h)))
        self.h = h
        cb.e._adopt(self)

    def clear(self):
        check(self.e.lib.somhip_distortion_clear(self.h))

    def accumulate(self, cb, ds, first=0, n=None):
        """data rows (first + s) % ds.n, s < n, against cb's rows as they are (somhip_distortion_accumulate)"""
        n = ds.n if n is None else n
        check(self.e.lib.somhip_distortion_accumulate(self.h, cb.h, ds.h, first, n))

    def evaluate(self, cb, r, units=True):
        """(totals, e): totals = {"energy", "scale", "samples"} at radius r against cb's current rows -- the energy resolves
        about 2^-52 * scale -- and e = float64[cb.n], the energy per unit (None with units=False)
        (somhip_distortion_evaluate)"""
        e = np.zeros(self.n, dtype=np.float64) if units else None
        tot = _lib.DistortionTotals()
        check(self.e.lib.somhip_distortion_evaluate(self.h, cb.h, float(np.float32(r)), _p(e, _lib.c_double_p), C.byref(tot)))
        return _distortion_totals(tot), e

    def read(self):
        """(hits uint32[n], sums float64[n, dim], sq float64[n]): the state as it stands (somhip_distortion_read)"""
        hits = np.zeros(self.n, dtype=np.uint32)
        sums = np.zeros((self.n, self.dim), dtype=np.float64)
        sq = np.zeros(self.n, dtype=np.float64)
        check(self.e.lib.somhip_distortion_read(self.h, _p(hits, _lib.c_u32_p), _p(sums, _lib.c_double_p), _p(sq, _lib.c_double_p)))
        return hits, sums, sq

    def close(self):
        if self.h and self.e.h:
            self.e.lib.somhip_distortion_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def map_distortion(cb, ds, r, first=0, n=None, units=True):
    """The distortion of a map over data rows (first + s) % ds.n, s < n, at radius r in one call: a Distortion made,
    accumulated, evaluated and closed.  Returns (totals, e) as Distortion.evaluate does."""
    st = Distortion(cb)
    try:
        st.accumulate(cb, ds, first, n)
        return st.evaluate(cb, r, units)
    finally:
        st.close()


def distortion_evaluate(cb, r, hits, sums, sq, units=True):
    """The evaluate stage alone on host-supplied per-unit hits, sums and squared-norm sums
    (somhip_debug_distortion_evaluate): (totals, e) as Distortion.evaluate gives them"""
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    sq = np.ascontiguousarray(sq, dtype=np.float64)
    assert hits.shape == (cb.n,) and sums.shape == (cb.n, cb.dim) and sq.shape == (cb.n,)
    e = np.zeros(cb.n, dtype=np.float64) if units else None
    tot = _lib.DistortionTotals()
    check(cb.e.lib.somhip_debug_distortion_evaluate(cb.h, float(np.float32(r)), _p(hits, _lib.c_u32_p), _p(sums, _lib.c_double_p),
                                                    _p(sq, _lib.c_double_p), _p(e, _lib.c_double_p), C.byref(tot)))
    return _distortion_totals(tot), e


def device_ptrs(cb, ds):
    """(tiles, rows, mask) device addresses of a codebook and a data set (somhip_debug_device_ptrs; mask 0: none): what
    the cached graph of online SOM iterations is keyed by."""
    out = (C.c_uint64 * 3)()
    check(cb.e.lib.somhip_debug_device_ptrs(cb.h, ds.h, out))
    return int(out[0]), int(out[1]), int(out[2])


def mapset_plan(n_rows, dim, masked=False, lib=None):
    """What a map set of this shape would be (somhip_debug_mapset_plan; host arithmetic, no GPU): a dict of whether its
    LDS image fits the budget, the workgroup's threads, units per thread, LDS bytes and the iterations per launch."""
    lib = lib or _lib.load()
    out = (C.c_int32 * 8)()
    check(lib.somhip_debug_mapset_plan(n_rows, dim, int(bool(masked)), out))
    return {"fits": bool(out[0]), "threads": out[1], "units_per_thread": out[2], "lds_bytes": out[3], "chunk": out[4],
            "masked": bool(out[5])}


class MapSet:
    """Many maps of one shape on the device (somhip_mapset): rows[T, n, d]; every map is trained as som_train(batch=1)
    would train a Codebook of its rows, all of them at once, each in one workgroup's LDS."""

    def __init__(self, engine, rows, topol, neigh, xdim, ydim):
        self.e = engine
        rows = _arr(rows, np.float32)
        assert rows.ndim == 3, "rows[T, n, d]"
        self.n_maps, self.n, self.dim = rows.shape
        self.topol, self.neigh, self.xdim, self.ydim = topol, neigh, xdim, ydim
        h = C.c_void_p()
        check(engine.lib.somhip_mapset_create(engine.h, _p(rows, _lib.c_float_p), self.n_maps, self.n, self.dim, topol, neigh,
                                              xdim, ydim, C.byref(h)))
        self.h = h
        engine._adopt(self)

    def train(self, ds, length, alpha, radius, alpha_type=ALPHA_LINEAR, use_fixed=0, use_weights=0, start_iter=0, count=None,
              data_first=None, trace=False):
        """som_training, batch 1, for every map; (trace_index, trace_diff) [T, count], or (None, None)."""
        count = length - start_iter if count is None else count
        data_first = start_iter % ds.n if data_first is None else data_first
        p = SomParams(length, alpha, radius, alpha_type, use_fixed, use_weights, 1, start_iter, count, data_first)
        ti = np.empty((self.n_maps, count), dtype=np.int32) if trace else None
        td = np.empty((self.n_maps, count), dtype=np.float32) if trace else None
        check(self.e.lib.somhip_mapset_train(self.h, ds.h, C.byref(p), _p(ti, _lib.c_i32_p), _p(td, _lib.c_float_p)))
        return ti, td

    def winners(self, ds, first=0, count=None):
        """find_winner_euc of data rows [first, first + count) against every map: (index, diff, ret) [T, count]."""
        count = ds.n if count is None else count
        idx = np.empty((self.n_maps, count), dtype=np.int32)
        diff = np.empty((self.n_maps, count), dtype=np.float32)
        ret = np.empty((self.n_maps, count), dtype=np.int32)
        check(self.e.lib.somhip_mapset_winners(self.h, ds.h, first, count, _p(idx, _lib.c_i32_p), _p(diff, _lib.c_float_p),
                                               _p(ret, _lib.c_i32_p)))
        return idx, diff, ret

    def download(self, first_map=0, n_maps=None):
        n_maps = self.n_maps - first_map if n_maps is None else n_maps
        out = np.empty((n_maps, self.n, self.dim), dtype=np.float32)
        check(self.e.lib.somhip_mapset_download(self.h, first_map, n_maps, _p(out, _lib.c_float_p)))
        return out

    def upload(self, rows, first_map=0):
        rows = _arr(rows, np.float32)
        assert rows.ndim == 3 and rows.shape[1:] == (self.n, self.dim)
        check(self.e.lib.somhip_mapset_upload(self.h, first_map, rows.shape[0], _p(rows, _lib.c_float_p)))

    def close(self):
        if self.h and self.e.h:
            self.e.lib.somhip_mapset_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BATCH_AUTO = -1          # somhip.h SOMHIP_BATCH_AUTO: the engine's own mini-batch sizes along the schedule


def som_auto_batch(lib, length, it, alpha=0.05, radius=128.0, n_units=65536, topol=TOPOL_HEXA, neigh=NEIGH_BUBBLE,
                   alpha_type=ALPHA_LINEAR):
    """(start, length) of the SOMHIP_BATCH_AUTO batch that holds iteration `it` of a run of `length` iterations with these
    parameters on a map of n_units units (somhip_som_auto_batch: a rule in (units, radius(t), alpha(t)); (it, 1) where the
    rule does not vouch for mini-batches); defaults = configs[3]"""
    a, b = C.c_int64(0), C.c_int64(0)
    p = SomParams(length, alpha, radius, alpha_type, 0, 0, BATCH_AUTO, 0, 0, 0)
    check(lib.somhip_som_auto_batch(C.byref(p), n_units, topol, neigh, it, C.byref(a), C.byref(b)))
    return a.value, b.value


def lvq_train(cb, ds, kind, length, alpha, alpha_type=ALPHA_LINEAR, winlen=0.0, epsilon=0.0,
              talpha=None, start_iter=0, count=None, data_first=None, trace=True):
    """lvq1/olvq1/lvq2/lvq3_training (reference lvq_rout.c:498-916).

    A masked data set (Dataset(..., mask=...)) runs in the exact batched engine like an unmasked one (the sample's
    mask in distance and update, lvq_pak.c:179-186, 343-347; whatever the rows store at masked positions is never
    read into a result); a run that visits a row with every component masked raises before training."""
    count = length - start_iter if count is None else count
    data_first = start_iter % ds.n if data_first is None else data_first
    knn = 2 if kind in (LVQ2, LVQ3) else 1
    p = LvqParams(kind, length, alpha, alpha_type, winlen, epsilon, start_iter, count, data_first)
    if kind == OLVQ1:
        talpha = (np.full(cb.n, alpha, dtype=np.float32) if talpha is None
                  else np.ascontiguousarray(talpha, dtype=np.float32).copy())
    ti = np.empty(count * knn, dtype=np.int32) if trace else None
    td = np.empty(count * knn, dtype=np.float32) if trace else None
    check(cb.e.lib.somhip_lvq_train(cb.h, ds.h, C.byref(p), _p(talpha, _lib.c_float_p),
                                    _p(ti, _lib.c_i32_p), _p(td, _lib.c_float_p)))
    return talpha, ti, td


LVQ_PAIRS = ("masked", "mfma", "direct")


def lvq_plan(cb, ds, kind, length, alpha, alpha_type=ALPHA_LINEAR, winlen=0.0, epsilon=0.0, start_iter=0, count=None,
             data_first=None, trace=True):
    """The plan lvq_train would follow with these arguments under the current environment (somhip_debug_lvq_plan; host
    arithmetic, no GPU work): a dict of the engine, the batched loop's form and the choices of a batch."""
    count = length - start_iter if count is None else count
    data_first = start_iter % ds.n if data_first is None else data_first
    p = LvqParams(kind, length, alpha, alpha_type, winlen, epsilon, start_iter, count, data_first)
    out = (C.c_int32 * 8)()
    check(cb.e.lib.somhip_debug_lvq_plan(cb.h, ds.h, C.byref(p), int(trace), out))
    return {"engine": "batched" if out[0] else "online", "loop": "nowait" if out[1] else "careful", "single": bool(out[2]),
            "pairs": LVQ_PAIRS[out[3]], "masked": bool(out[4]), "knn": out[5], "slots": out[6], "dyn_lds": out[7]}


LVQ_BMAX, LVQ_AW = 1024, 32     # samples per batch of the exact batched engine; adjacency words per sample


def lvq_relation(cb, ds, kind, length, alpha, alpha_type=ALPHA_LINEAR, winlen=0.0, epsilon=0.0, start_iter=0, data_first=0,
                 count=1):
    """The front and the relation of one batch of the exact batched engine (somhip_debug_lvq_relation): iterations
    [start_iter, start_iter + count) on data rows data_first, data_first + 1, ... (mod n), made as lvq_train makes them
    under the current environment; nothing is trained.  A dict of numpy arrays: keys [count, 8] uint64, rho [count],
    xnorm [count], amax (float32 scalar; < 0: unknown), adj [count, 32] uint32, ncomp, start [ncomp + 1],
    comp_samples [count].  OLVQ1 reads the rates of lvq_rates_upload."""
    p = LvqParams(kind, length, alpha, alpha_type, winlen, epsilon, start_iter, count, data_first)
    n = max(int(count), 0)
    keys = np.zeros((n, 8), dtype=np.uint64)
    rho, xnorm = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    amax = np.zeros(1, dtype=np.float32)
    adj = np.zeros((n, LVQ_AW), dtype=np.uint32)
    ncomp, start, comp = np.zeros(1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    check(cb.e.lib.somhip_debug_lvq_relation(cb.h, ds.h, C.byref(p), data_first, count, _p(keys, _lib.c_u64_p),
                                             _p(rho, _lib.c_float_p), _p(xnorm, _lib.c_float_p), _p(amax, _lib.c_float_p),
                                             _p(adj, _lib.c_u32_p), _p(ncomp, _lib.c_i32_p), _p(start, _lib.c_i32_p),
                                             _p(comp, _lib.c_i32_p)))
    nc = int(ncomp[0])
    return {"keys": keys, "rho": rho, "xnorm": xnorm, "amax": amax[0], "adj": adj, "ncomp": nc,
            "start": start[:max(0, min(nc, n)) + 1].copy(), "comp_samples": comp}


def lvq_components(eng, adj, count, single=False):
    """k_lvq_components alone on adjacency rows adj [count, 32] uint32 (somhip_debug_lvq_components):
    (ncomp, start [ncomp + 1], comp_samples [count])."""
    n = max(int(count), 0)
    adj = np.ascontiguousarray(adj, dtype=np.uint32)
    if adj.shape != (n, LVQ_AW):
        raise ValueError("lvq_components: adj must be [count, %d]" % LVQ_AW)
    ncomp, start, comp = np.zeros(1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    check(eng.lib.somhip_debug_lvq_components(eng.h, _p(adj, _lib.c_u32_p), count, int(single), _p(ncomp, _lib.c_i32_p),
                                              _p(start, _lib.c_i32_p), _p(comp, _lib.c_i32_p)))
    nc = int(ncomp[0])
    return nc, start[:max(0, min(nc, n)) + 1].copy(), comp


def lvq_rates_upload(cb, talpha):
    """OLVQ1's per-row rates to the device (somhip_lvq_rates_upload)."""
    ta = np.ascontiguousarray(talpha, dtype=np.float32)
    if ta.shape != (cb.n,):
        raise ValueError("lvq_rates_upload: one rate per code row (%d)" % cb.n)
    check(cb.e.lib.somhip_lvq_rates_upload(cb.h, _p(ta, _lib.c_float_p)))


def qerror_sum(diff, ret=None):
    """find_qerror's accumulation (reference som_rout.c:698-715): a float32 running sum of
    double square roots in data order -- O(n) host work on the winners the GPU returned."""
    q = np.float32(0.0)
    d = np.asarray(diff, dtype=np.float32).reshape(-1)
    for i in range(d.shape[0]):
        if ret is not None and not ret[i]:
            continue
        q = np.float32(np.float64(q) + np.sqrt(np.float64(d[i])))
    return q


def qerror2_sum(cb, ds, radius, first=0, count=None):
    """find_qerror2 (reference som_rout.c:823-885): per-sample neighbourhood-weighted errors from
    the GPU, added in data order into a float32 accumulator like the reference's."""
    n = ds.n if count is None else count
    out = np.zeros(n, dtype=np.float32)
    ret = np.zeros(n, dtype=np.int32)
    check(cb.e.lib.somhip_qerror2(cb.h, ds.h, C.c_float(radius), first, n, _p(out, _lib.c_float_p),
                                  _p(ret, _lib.c_i32_p)))
    q = np.float32(0.0)
    for i in range(n):
        if ret[i]:
            q = np.float32(q + out[i])
    return q


def class_nearest_later(ds):
    """Per row of a labelled data set: (min_sq, state) of somhip_class_nearest_later -- the squared distance (the
    reference's fp32 sum, bit for bit) to the nearest LATER row of the same label, and 0 = no later row of the label,
    1 = min_sq valid, 2 = some later row of the label shares no unmasked component with the row (distance -1).
    The inner loop of med_distances (lvq_rout.c:384-491); the distance is float32(sqrt(float64(min_sq)))."""
    min_sq = np.empty(ds.n, dtype=np.float32)
    state = np.empty(ds.n, dtype=np.int32)
    check(ds.e.lib.somhip_class_nearest_later(ds.h, _p(min_sq, _lib.c_float_p), _p(state, _lib.c_i32_p)))
    return min_sq, state


def umatrix(cb, average=False, median=False):
    """The U-matrix of a whole hexa / rect map from the rows on the device (somhip_umatrix): (u, (min, max)).
    u is float32 [2 ydim - 1, 2 xdim - 1], u[y, x] = SOM_PAK's uvalue[x][y] after calc_umatrix (map.c:130-500), then
    average_umatrix and median_umatrix when asked for, bit for bit; min and max are those of map.c:474-485, before
    the scaling to [0, 1].  Raises on a codebook that is not a map, on a shard, on a side below 2 and on max == min."""
    u = np.empty((max(2 * cb.ydim - 1, 1), max(2 * cb.xdim - 1, 1)), dtype=np.float32)
    mm = np.zeros(2, dtype=np.float64)
    check(cb.e.lib.somhip_umatrix(cb.h, (UMAT_AVERAGE if average else 0) | (UMAT_MEDIAN if median else 0),
                                  _p(u, _lib.c_float_p), _p(mm, _lib.c_double_p)))
    return u, (float(mm[0]), float(mm[1]))


def planes(cb, first=0, count=None):
    """Grey-scaled component planes of a whole codebook from the rows on the device (somhip_planes): (grey, lo, hi).
    grey is float32 [count, n], grey[j, k] = SOM_PAK's cv (planes.c:172-176) of component first + j of row k, bit for
    bit; lo and hi are float32 [count], the component's minval and maxval over the rows.  count=None: every component
    from `first` on.  Raises on a shard and on a window outside [0, dim)."""
    count = cb.dim - first if count is None else count
    grey = np.empty((max(count, 0), cb.n), dtype=np.float32)
    lo = np.empty(max(count, 0), dtype=np.float32)
    hi = np.empty(max(count, 0), dtype=np.float32)
    check(cb.e.lib.somhip_planes(cb.h, first, count, _p(grey, _lib.c_float_p), _p(lo, _lib.c_float_p),
                                 _p(hi, _lib.c_float_p)))
    return grey, lo, hi


def sammon_zero_pairs(cb):
    """The pairs of rows (i, j), i < j, at reference distance 0.0 (somhip_sammon_zero_pairs): int64 [n, 2], sorted --
    what sammon's remove_identicals (sammon.c:84-128) asks.  Distance 0 is not row equality: small squares underflow."""
    n = C.c_int64(0)
    cap = 16 * cb.n
    pairs = np.empty((cap, 2), dtype=np.uint32)
    check(cb.e.lib.somhip_sammon_zero_pairs(cb.h, _p(pairs, _lib.c_u32_p), cap, C.byref(n)))
    if n.value > cap:                      # many identical rows: once more with room for all
        cap = n.value
        pairs = np.empty((cap, 2), dtype=np.uint32)
        check(cb.e.lib.somhip_sammon_zero_pairs(cb.h, _p(pairs, _lib.c_u32_p), cap, C.byref(n)))
    return pairs[:n.value].astype(np.int64)


def sammon(cb, x0, y0, rlen, want_error=False):
    """rlen iterations of SOM_PAK's Sammon mapping (sammon.c:187-225) of the codebook's rows from the initial table
    (x0, y0), bit for bit: (x, y), and with want_error the mapping error after every iteration (float64 [rlen]; summed
    by a tree, so close to the reference's fp32 running sum, not bit-equal).  Raises on a codebook with fewer than 2
    rows or with a pair of rows at distance 0 (sammon_zero_pairs lists them)."""
    x = np.ascontiguousarray(x0, dtype=np.float32).copy()
    y = np.ascontiguousarray(y0, dtype=np.float32).copy()
    if x.shape != (cb.n,) or y.shape != (cb.n,):
        raise ValueError("sammon: the initial table must have one x and one y per row (%d)" % cb.n)
    err = np.zeros(rlen, dtype=np.float64) if want_error else None
    check(cb.e.lib.somhip_sammon(cb.h, rlen, _p(x, _lib.c_float_p), _p(y, _lib.c_float_p), _p(err, _lib.c_double_p)))
    return (x, y, err) if want_error else (x, y)
