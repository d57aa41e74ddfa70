"""Constructed inputs for the binned unordered push (glint_amd/csrc/glint_bin.hip) and a host model of
what its kernels do with them. Plain numpy: no GPU, no product code.

Which code runs inside bin_scan, bin_fsort, bin_plan and bin_apply2 depends on where a push's records
fall. For the plain front end (GLINT_BIN_FRONT=prep) that is deterministic up to the order inside one
chunk's run: chunk c is records [c kchunk, (c + 1) kchunk) of the push, a bucket's records are its runs in
chunk order, item j of a bucket is records [j item, (j + 1) item) of that order. So this module

* restates bin_layout / bin_geometry (``layout``; tests/test_bin_cases_cpu.py holds it against the real
  headers through tests/c/plan_probe.cpp),
* models a push (``model``): the buckets' totals and items, every item's chunk window exactly, bounds on
  the records of each (item, slab) pair that hold for any order inside a run, the plan's choices that
  follow from them (wave emit or walk, staging tiles, groups of sparse slabs, the units of a slab), and
* builds cases (``CASES``) whose keys provably reach the data-dependent branches, each with the
  predicates over the model that say so (``Case.checks``).

tests/test_gpu_binned_shapes.py pushes the cases on the device and compares the sums with the oracle.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# ---- constants restated from the sources (file:line of the definition) ---------------------------------
K_SLAB_BITS = 12          # glint_bin_plan.h:15  GLINT_SLAB_BITS
K_SLAB = 1 << K_SLAB_BITS  # glint_bin_plan.h:18
K_ATPB = 1024             # glint_bin_plan.h:21  GLINT_PART_TPB
K_APER = 4                # glint_bin_plan.h:25  GLINT_PART_PER
K_APER_PLAIN = 8          # glint_bin_plan.h:29  GLINT_PART_PER_PLAIN
K_PART_WPC = 1            # glint_bin_plan.h:37-41  kPartWgPerCuDedup / kPartWgPerCuPlain at kATPB == 1024
K_STPB = 1024             # glint_bin_plan.h:44  GLINT_FSORT_TPB
K_SPER = 12               # glint_bin_plan.h:54,57  GLINT_FSORT_PER_SMALL == GLINT_FSORT_PER_LARGE
K_RUN_MAX = 128           # glint_bin_plan.h:61
K_UNIT_CAP = 4096         # glint_bin_plan.h:63  GLINT_UNIT_CAP
K_HOT_SLOTS = 2048        # glint_bin_plan.h:67
K_WIDE_SLOTS = 8192       # glint_bin_plan.h:68
K_COARSE_BITS_MIN = 7     # glint_bin_plan.h:83  GLINT_BIN_CB
K_PLAN_SPLIT = 2          # glint_bin.hip:1114  GLINT_PLAN_SPLIT
K_SPARSE_MAX2 = 1024      # glint_bin.hip:1119,1124  kSparseCap2 == kSparseMax2
K_LIST_MAX = 768          # glint_bin.hip:1125
K_PLAN_LDS, K_PLAN_PTAB = 65536, 16640             # glint_bin.hip:1142
K_PLAN_LDS_FUSED, K_PLAN_PTAB_FUSED = 32768, 8320  # glint_bin.hip:1143
K_GROUP_SLAB_AVG = 512    # glint_bin.hip:1146  GLINT_GROUP_SLAB_AVG
K_GROUP_CAP = 2048        # glint_bin.hip:1148
K_GROUP_MAX = 16          # glint_bin.hip:1150
K_FWIN = 2048             # glint_bin.hip:1423
K_APPLY2_OCC = 4          # glint_bin.hip:1627  GLINT_APPLY2_WAVES: resident bin_apply2 workgroups per CU

SCALARS = ("small_push", "per", "kchunk", "nchunks_max", "wpc", "G", "item", "max_fitems", "max_units", "nstride",
           "ctstride", "fb", "nb", "nf", "nslab")
BUFFERS = ("ct", "P", "Q", "Bb", "Ib", "fitems", "cwin", "off2", "units", "runs", "hot_tags", "wpart", "addr_a",
           "val_a", "val_b", "e_b")
LAYOUT_WORDS = SCALARS + BUFFERS + ("need",)  # plan_probe.cpp plan_layout's output, in its order


def _pad256(b):
    return (b + 255) & ~255


def geometry(elems, cbmin):
    """bin_geometry (glint_bin_plan.h:86): fb, nb, nf, nslab"""
    slabs = (elems + K_SLAB - 1) // K_SLAB
    sb = 0
    while (1 << sb) < slabs:
        sb += 1
    cb = min(sb, max(cbmin, sb - 10 if sb > 10 else 0))
    fb = sb - cb
    return fb, 1 << cb, 1 << fb, (1 << cb) << fb


def layout(elems, n, cus, front, acc_bytes=8, hot_occ=1, apply2_occ=K_APPLY2_OCC):
    """bin_layout (glint_bin_plan.h:162) word for word, and push_binned's bin_apply2 grid and unit order
    (glint_bin.hip:2108-2111). front: 0 plain, 1 plain + hot split, 2 chunk dedup."""
    L = {}
    small = geometry(elems, K_COARSE_BITS_MIN)[1] + n // (K_STPB * K_SPER) + 1 <= 4 * cus
    L["small_push"] = int(small)
    per = K_APER_PLAIN if front == 0 and not small else K_APER
    L["per"] = per
    fb, nb, nf, nslab = geometry(elems, K_COARSE_BITS_MIN if per == K_APER_PLAIN else K_COARSE_BITS_MIN - 1)
    kchunk = K_ATPB * per
    nch = (n + kchunk - 1) // kchunk
    wpc = K_PART_WPC if front != 1 else min(K_PART_WPC, hot_occ)
    G = max(1, min(nch, cus * wpc))
    item = K_STPB * K_SPER
    max_fitems = nb + n // item + 1
    max_units = nslab + n // K_UNIT_CAP + min(n, max_fitems * nf) // K_RUN_MAX + 1
    L.update(kchunk=kchunk, nchunks_max=nch, wpc=wpc, G=G, item=item, max_fitems=max_fitems, max_units=max_units,
             nstride=nch, ctstride=nch + 1, fb=fb, nb=nb, nf=nf, nslab=nslab)
    sizes = (("ct", (nch + 1) * nb * 4), ("P", nb * (nch + 1) * 4), ("Q", nb * nch * 4), ("Bb", nb * 4), ("Ib", nb * 4),
             ("fitems", max_fitems * 8), ("cwin", max_fitems * 8), ("off2", max_fitems * (nf + 1) * 4),
             ("units", max_units * 16), ("runs", max_units * K_RUN_MAX * 8), ("hot_tags", K_HOT_SLOTS * 4),
             ("wpart", G * K_WIDE_SLOTS * acc_bytes if front == 1 else 0), ("addr_a", n * 4), ("val_a", n * acc_bytes),
             ("val_b", n * acc_bytes), ("e_b", n * 2))
    cur = 0
    for name, nbytes in sizes:
        L[name] = cur
        cur += _pad256(nbytes)
    L["need"] = cur
    L["apply2_grid"] = min(max_units, cus * apply2_occ)
    L["xcd_map"] = int(L["apply2_grid"] % 8 == 0)
    return L


def plan_shape(L):
    """Where a bucket is planned: (slab ranges of its planning workgroups, bytes of staged rows, ptab
    entries). A small push plans inside bin_fsort (glint_bin.hip:1495), a large one in bin_plan
    (glint_bin.hip:1367-1370)."""
    nf = L["nf"]
    if L["small_push"]:
        return [(0, nf)], K_PLAN_LDS_FUSED, K_PLAN_PTAB_FUSED
    fs = max(64, nf // K_PLAN_SPLIT)
    return [(s * fs, min(nf, (s + 1) * fs)) for s in range(K_PLAN_SPLIT) if s * fs < nf], K_PLAN_LDS, K_PLAN_PTAB


# ---- the model ---------------------------------------------------------------------------------------
@dataclass
class Model:
    L: dict
    group_on: bool
    addr: np.ndarray
    H: np.ndarray        # [nb, nf] records per slab (exact)
    T: np.ndarray        # [nb] records per bucket
    J: np.ndarray        # [nb] fine items per bucket, max(1, ceil(T / item))
    Ib: np.ndarray       # [nb] the model's number of a bucket's item 0 (buckets in order; the device's is any)
    cwx: np.ndarray      # [items] chunk of the item's first record (exact)
    cwy: np.ndarray      # [items] chunk of its last record (exact)
    lo: np.ndarray       # [items, nf] records of the (item, slab) pair at least ...
    hi: np.ndarray       # ... and at most, whatever the order inside each chunk's run
    jt: int              # items per staged tile of the plan
    wave: np.ndarray     # [nb] the plan of the bucket takes the wave emit (else the walk)
    span: np.ndarray     # [nb, nf] 1 a slab planned alone, gs the leader of a group of gs slabs, 0 a member
    _distinct: np.ndarray = field(default=None, repr=False)

    @property
    def chunk_span(self):
        return self.cwy - self.cwx + 1

    def item(self, b, j):
        return int(self.Ib[b]) + j

    @property
    def distinct(self):
        """[nb, nf] distinct elements touched per slab"""
        if self._distinct is None:
            u = np.unique(self.addr)
            nslab = self.L["nb"] * self.L["nf"]
            self._distinct = np.bincount(u >> K_SLAB_BITS, minlength=nslab).reshape(self.L["nb"], self.L["nf"])
        return self._distinct

    def exact(self, b, f, width=1):
        r = slice(int(self.Ib[b]), int(self.Ib[b] + self.J[b]))
        return bool((self.lo[r, f:f + width] == self.hi[r, f:f + width]).all())

    def units(self, b, f):
        """The apply units of the slab (or of the group that slab f leads) as (runs, records, closed_by)
        with closed_by in {"cap", "runs", "end"}; None when they depend on the order inside a run.
        plan_bucket's wave emit (glint_bin.hip:1333-1343) or walk (glint_bin.hip:1211-1249)."""
        sp = int(self.span[b, f])
        if sp == 0:
            return []
        if not self.exact(b, f, sp):
            return None
        r = slice(int(self.Ib[b]), int(self.Ib[b] + self.J[b]))
        counts = self.lo[r, f:f + sp].sum(axis=1)
        tot = int(counts.sum())
        if tot == 0:
            return []
        if self.wave[b]:
            if sp > 1:
                return [(int((counts > 0).sum()), tot, "end")]
            pre = np.concatenate(([0], np.cumsum(counts)))
            out = []
            for u in range(-(-tot // K_UNIT_CAP)):
                lo_, hi_ = u * K_UNIT_CAP, min(tot, (u + 1) * K_UNIT_CAP)
                nr = int(((counts > 0) & (pre[:-1] < hi_) & (pre[1:] > lo_)).sum())
                out.append((nr, hi_ - lo_, "cap" if hi_ - lo_ == K_UNIT_CAP else "end"))
            return out
        out, acc, nr = [], 0, 0
        for c in counts:
            c = int(c)
            while c:
                take = min(c, K_UNIT_CAP - acc)
                acc += take
                c -= take
                nr += 1
                if acc == K_UNIT_CAP or nr == K_RUN_MAX:
                    out.append((nr, acc, "cap" if acc == K_UNIT_CAP else "runs"))
                    acc = nr = 0
        if acc:
            out.append((nr, acc, "end"))
        return out


def model(addr, L, group_on=True):
    """The plain front end's push of the records at shard-local element addresses `addr`, in this order."""
    addr = np.ascontiguousarray(addr, np.int64)
    n = addr.size
    kchunk, item, nb, nf, fb, nch = L["kchunk"], L["item"], L["nb"], L["nf"], L["fb"], L["nchunks_max"]
    assert n > 0 and nch == -(-n // kchunk) and kchunk < item
    slab = addr >> K_SLAB_BITS
    assert 0 <= int(slab.min()) and int(slab.max()) < nb * nf
    H = np.bincount(slab, minlength=nb * nf).reshape(nb, nf)
    T = H.sum(axis=1)
    J = np.maximum(1, -(-T // item))
    Ib = np.concatenate(([0], np.cumsum(J)[:-1]))
    Bb = np.concatenate(([0], np.cumsum(T)[:-1]))  # the model's bucket order: by number
    # (bucket, chunk, slab) triples with their counts, sorted; a run = the triples of one (bucket, chunk)
    code = ((slab >> fb) * nch + np.arange(n, dtype=np.int64) // kchunk) * nf + (slab & (nf - 1))
    u, c = np.unique(code, return_counts=True)
    del code
    rc, tf = u // nf, u % nf
    first = np.flatnonzero(np.concatenate(([True], rc[1:] != rc[:-1])))
    run_cnt = np.add.reduceat(c, first)
    run_b, run_c = rc[first] // nch, rc[first] % nch
    g0 = np.cumsum(run_cnt) - run_cnt  # the run's first record, counting through the buckets in order
    P = g0 - Bb[run_b]                 # ... and within its bucket: bin_scan's P[b][c]
    # every item's chunk window (bin_scan's cwin): the runs holding its first and last records
    nitems = int(J.sum())
    it_b = np.repeat(np.arange(nb), J)
    it_j = np.arange(nitems) - Ib[it_b]
    empty = T[it_b] == 0
    rec0 = Bb[it_b] + it_j * item
    rec1 = Bb[it_b] + np.minimum(T[it_b], (it_j + 1) * item) - 1
    rx = np.clip(np.searchsorted(g0, rec0, "right") - 1, 0, g0.size - 1)
    ry = np.clip(np.searchsorted(g0, rec1, "right") - 1, 0, g0.size - 1)
    cwx = np.where(empty, 0, run_c[rx])
    cwy = np.where(empty, 0, run_c[ry])
    # records of each (item, slab) pair: a run inside one item gives all of its slab counts to that item;
    # a run cut by an item boundary (at most one: kchunk < item) gives the item that takes o of its cnt
    # records between max(0, c - (cnt - o)) and min(c, o) of a slab's c
    tr = np.repeat(np.arange(first.size), np.diff(np.concatenate((first, [u.size]))))
    tP, tcnt, tb = P[tr], run_cnt[tr], run_b[tr]
    j0, j1 = tP // item, (tP + tcnt - 1) // item
    assert int((j1 - j0).max()) <= 1
    o0 = np.where(j1 > j0, (j0 + 1) * item - tP, tcnt)
    lo = np.zeros(nitems * nf)
    hi = np.zeros(nitems * nf)
    for jj, o in ((j0, o0), (j1, tcnt - o0)):
        sel = o > 0
        flat = (Ib[tb[sel]] + jj[sel]) * nf + tf[sel]
        hi += np.bincount(flat, np.minimum(c[sel], o[sel]), minlength=nitems * nf)
        lo += np.bincount(flat, np.maximum(0, c[sel] - (tcnt[sel] - o[sel])), minlength=nitems * nf)
    lo = lo.astype(np.int64).reshape(nitems, nf)
    hi = hi.astype(np.int64).reshape(nitems, nf)
    # the plan (plan_bucket, glint_bin.hip:1186-1187, 1258-1259, 1278-1286)
    ranges, rowb, ptab = plan_shape(L)
    nl = ranges[0][1] - ranges[0][0] + 1
    jt = rowb // 2 // nl
    wave = (J <= 64) & (J <= jt) & (J * nl <= ptab)
    span = np.ones((nb, nf), np.int64)
    if group_on:
        gs = 2
        while gs <= K_GROUP_MAX and gs <= nf:
            s = np.repeat(H.reshape(nb, nf // gs, gs).sum(axis=2), gs, axis=1)
            span[(s > 0) & (s <= min(K_GROUP_CAP, gs * K_GROUP_SLAB_AVG))] = gs
            gs *= 2
        span[J > K_RUN_MAX, :] = 1
        f = np.arange(nf)[None, :]
        span[(span > 1) & ((f & (span - 1)) != 0)] = 0
    return Model(L=L, group_on=group_on, addr=addr, H=H, T=T, J=J, Ib=Ib, cwx=cwx, cwy=cwy, lo=lo, hi=hi, jt=jt,
                 wave=wave, span=span)


# ---- predicates: one per branch ------------------------------------------------------------------------
def slow_items(m):
    """items gathered by bin_fsort's pos_slow: a chunk window wider than kFWin (glint_bin.hip:1465)"""
    return set(np.flatnonzero(m.chunk_span > K_FWIN).tolist())


def wave_emit(m):
    """non-empty buckets planned by the wave emit (glint_bin.hip:1259)"""
    return set(np.flatnonzero(m.wave & (m.T > 0)).tolist())


def walk_buckets(m):
    return set(np.flatnonzero(~m.wave & (m.T > 0)).tolist())


def walk_multitile(m):
    """buckets whose off2 rows are staged again tile by tile for the emit pass: the walk with J > jt
    (glint_bin.hip:1215)"""
    return set(np.flatnonzero(~m.wave & (m.T > 0) & (m.J > m.jt)).tolist())


def grouped(m, gs):
    """(bucket, slab) leaders of a group of gs sparse slabs (glint_bin.hip:1281-1285)"""
    return set(zip(*np.nonzero(m.span == gs)))


def _singles(m, cond):
    """(bucket, slab) of slabs planned alone whose units are known and satisfy cond(units)"""
    out = set()
    for b, f in zip(*np.nonzero((m.span == 1) & (m.H > 0))):
        un = m.units(b, f)
        if un is not None and cond(un):
            out.add((int(b), int(f)))
    return out


def runcap_slabs(m):
    """slabs with a unit closed at kRunMax runs before kUnitCap records (glint_bin.hip:1234)"""
    return _singles(m, lambda un: any(why == "runs" and acc < K_UNIT_CAP for _, acc, why in un))


def shared_slab(m):
    """slabs cut into two or more units: flushed with device atomics (glint_bin.hip:1902)"""
    return _singles(m, lambda un: len(un) >= 2)


def excl_full(m):
    """exclusive slabs of exactly kUnitCap records"""
    return _singles(m, lambda un: len(un) == 1 and un[0][1] == K_UNIT_CAP)


def _exclusive(m, pick):
    d = m.distinct
    return {(b, f) for b, f in _singles(m, lambda un: len(un) == 1) if pick(int(m.H[b, f]), int(d[b, f]))}


def sparse_list(m):
    """exclusive slabs written back through the touched list (glint_bin.hip:1750, 1824)"""
    return _exclusive(m, lambda h, d: h <= K_SPARSE_MAX2 and d <= K_LIST_MAX)


def sparse_to_sweep(m):
    """exclusive slabs that list their touched elements and then sweep: more than kListMax distinct"""
    return _exclusive(m, lambda h, d: h <= K_SPARSE_MAX2 and d > K_LIST_MAX)


def dense_sweep(m):
    """exclusive slabs above kSparseMax2 records: the whole-line sweep without a list"""
    return _exclusive(m, lambda h, d: h > K_SPARSE_MAX2)


# ---- cases ---------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    elems: int
    front: int               # the front end the model is claimed for
    addr: np.ndarray         # shard-local element addresses, in push order
    L: dict
    checks: object           # model -> {predicate: bool}
    cols: int = 0            # > 0: the same addresses as a matrix shard of rows x cols, pitch cols + 1

    @property
    def n(self):
        return int(self.addr.size)


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


def _slab_base(L, b, f):
    return ((b << L["fb"]) + f) << K_SLAB_BITS


def _in_slab(rng, L, b, f, count, width=K_SLAB):
    return _slab_base(L, b, f) + rng.integers(0, width, count)


def _chunk(rng, L, b, counts, heavy, kchunk=None):
    """One whole partition chunk of bucket b: counts[f] records in slab f, the rest spread over `heavy`"""
    parts = [_in_slab(rng, L, b, f, c) for f, c in counts.items() if c]
    rest = (kchunk or L["kchunk"]) - sum(counts.values())
    assert rest >= 0
    hs = rng.integers(0, len(heavy), rest)
    parts.append(_slab_base(L, b, 0) + (np.asarray(heavy)[hs] << K_SLAB_BITS) + rng.integers(0, K_SLAB, rest))
    return rng.permutation(np.concatenate(parts))


def _uniform_over(rng, L, buckets, count, elems):
    """count records uniform over the elements of `buckets` (below elems)"""
    per = K_SLAB << L["fb"]
    b = np.asarray(buckets)[rng.integers(0, len(buckets), count)]
    a = b * per + rng.integers(0, per, count)
    return np.minimum(a, elems - 1) if int(a.max()) >= elems else a


# A. long thin buckets: bin_fsort's pos_slow gather -------------------------------------------------------
A_ELEMS = 1 << 22
A_SPANS = (2047, 2048, 2049)


def case_a(cus, front=0):
    """One record per chunk in single-item buckets whose items span 2047, 2048 (the last fast span), 2049
    (the first slow one) and all chunks; a bucket whose item 0 is filled by the push's first chunks and
    whose item 1 then takes one record per chunk to the end (slow, v0 != 0, cw.x > 0). Every special
    record is on an element of its own, so the hot front end keeps it cold and its chunk is the same."""
    nchunks = 2304 if front == 0 else 2100
    per = K_APER_PLAIN if front == 0 else K_APER
    n = nchunks * K_ATPB * per
    L = layout(A_ELEMS, n, cus, front)
    rng = _rng(f"A{front}")
    kchunk, item, nb = L["kchunk"], L["item"], L["nb"]
    per_b = K_SLAB << L["fb"]
    thin = {1: A_SPANS[0], 2: A_SPANS[1], 3: A_SPANS[2], 4: nchunks}   # bucket -> chunks [first, first + span)
    first = {1: 5, 2: 17, 3: 40, 4: 0}
    fill_b = 5
    nfill = item // kchunk + 1  # the chunks that fill item 0 of bucket fill_b, evenly
    others = list(range(6, nb))
    own = {b: b * per_b + rng.permutation(per_b)[:item + nchunks] for b in list(thin) + [fill_b]}
    special = np.full((nchunks, len(thin) + 1), -1, np.int64)
    for k, (b, sp) in enumerate(thin.items()):
        cs = np.arange(first[b], first[b] + sp)
        special[cs, k] = own[b][cs]
    special[nfill:, -1] = own[fill_b][item + np.arange(nfill, nchunks)]
    chunks = []
    for c in range(nchunks):
        s = special[c][special[c] >= 0]
        if c < nfill:
            q = item // nfill
            s = np.concatenate((s, own[fill_b][c * q:(c + 1) * q]))
        rest = _uniform_over(rng, L, others, kchunk - s.size, A_ELEMS)
        chunks.append(rng.permutation(np.concatenate((s, rest))))
    addr = np.concatenate(chunks)

    def checks(m):
        sp = m.chunk_span
        slow = slow_items(m)
        want_slow = {m.item(3, 0), m.item(4, 0), m.item(fill_b, 1)}
        return {
            "chunks": L["nchunks_max"] == nchunks and L["kchunk"] == K_ATPB * per,
            "thin_single_items": all(m.J[b] == 1 for b in thin),
            "span_2047_2048_fast": [int(sp[m.item(b, 0)]) for b in (1, 2)] == [2047, 2048] and
            not ({m.item(1, 0), m.item(2, 0)} & slow),
            "span_2049_slow": int(sp[m.item(3, 0)]) == 2049,
            "span_all_slow": int(sp[m.item(4, 0)]) == nchunks,
            "fill_item0_full_in_first_chunks": int(m.J[fill_b]) == 2 and int(m.cwy[m.item(fill_b, 0)]) == nfill - 1,
            "fill_item1_slow_v0_cwx": int(m.cwx[m.item(fill_b, 1)]) == nfill and
            int(sp[m.item(fill_b, 1)]) == nchunks - nfill > K_FWIN,
            "slow_items": want_slow <= slow,
            "other_items_fast": all(int(sp[i]) <= K_FWIN for i in range(m.item(others[0], 0), sp.size)),
        }

    return Case(f"A_{'prep' if front == 0 else 'hot'}", A_ELEMS, front, addr, L, checks)


# B. item-count boundaries in the plan launch ------------------------------------------------------------
B_ELEMS = 1 << 22
B_CHUNKS = 1664
# slabs of a special bucket: heavy, empty, thin (8 per item), exactly 4096, exactly 4097, medium, one per
# item (a 2-group with its empty neighbour), empty
B_HEAVY, B_THIN, B_4096, B_4097, B_MED, B_ONE = 0, 2, 3, 4, 5, 6


def case_b(cus):
    """A large push (bin_plan runs; nf = 8, chunks of 8192 = 2/3 item). Buckets 1..4 get exactly 64 item,
    64 item + 1, 128 item and 129 item + 1 records in whole chunks of their own, so every second chunk
    boundary is an item boundary (bin_scan's runs end exactly at j item). Of three consecutive chunks of a
    bucket the first lies in item 2k, the third in item 2k + 1 and the second is cut between them: the thin
    slabs' records go to the first and third, so their counts per item are exact."""
    n = B_CHUNKS * K_ATPB * K_APER_PLAIN
    L = layout(B_ELEMS, n, cus, 0)
    rng = _rng("B")
    kchunk, item, nb = L["kchunk"], L["item"], L["nb"]
    items = {1: 64, 2: 64, 3: 128, 4: 129}
    extra = {2, 4}  # one record more, in the push's last chunk
    others = list(range(8, nb))
    chunks = []
    for b, ji in items.items():
        for k in range(ji * item // kchunk):
            counts = {B_MED: 100}
            if k % 3 != 1:
                counts.update({B_THIN: 8, B_ONE: 1})
            if k == 0:
                counts[B_4096] = K_UNIT_CAP
            if k == 2:
                counts[B_4097] = K_UNIT_CAP + 1
            chunks.append(_chunk(rng, L, b, counts, [B_HEAVY]))
    # the 129-item bucket's last half chunk, beside other buckets' records
    half = ji * item % kchunk
    assert half == kchunk // 2
    chunks.append(rng.permutation(np.concatenate((_in_slab(rng, L, 4, B_HEAVY, half),
                                                  _uniform_over(rng, L, others, kchunk - half, B_ELEMS)))))
    nspecial = sum(c.size for c in chunks)
    fill = _uniform_over(rng, L, others, n - nspecial - len(extra), B_ELEMS)
    last = np.concatenate((fill[-(kchunk - len(extra)):], [_slab_base(L, b, B_HEAVY) + 7 for b in sorted(extra)]))
    addr = np.concatenate(chunks + [fill[:-(kchunk - len(extra))], rng.permutation(last)])
    assert addr.size == n

    def checks(m):
        runcap, shared, full, g2 = runcap_slabs(m), shared_slab(m), excl_full(m), grouped(m, 2)
        return {
            "large_push": not L["small_push"] and L["kchunk"] == 8192 and L["nf"] == 8,
            "totals": [int(m.T[b]) for b in (1, 2, 3, 4)] == [64 * item, 64 * item + 1, 128 * item, 129 * item + 1],
            "items": [int(m.J[b]) for b in (1, 2, 3, 4)] == [64, 65, 128, 130],
            "wave_emit_64_only": 1 in wave_emit(m) and {2, 3, 4} <= walk_buckets(m),
            "last_item_one_record": all(int(m.hi[m.item(b, int(m.J[b]) - 1)].sum()) == 1 for b in (2, 4)),
            "item_boundary_on_chunk_boundary": all(
                int(m.cwy[m.item(b, 1)]) + 1 == int(m.cwx[m.item(b, 2)]) for b in (1, 2, 3, 4)),
            "thin_exact": all(m.exact(b, B_THIN) and m.exact(b, B_ONE) for b in (1, 2, 3, 4)),
            "runcap": {(3, B_THIN), (4, B_THIN), (4, B_ONE)} <= runcap,
            "runcap_shared": {(4, B_THIN), (4, B_ONE)} <= shared,
            "excl_full": {(b, B_4096) for b in (1, 2, 3, 4)} <= full,
            "cut_4097": {(b, B_4097) for b in (1, 2, 3, 4)} <= shared,
            "sparse_list": {(1, B_THIN), (2, B_THIN)} <= sparse_list(m),
            "group2_wave_and_walk": {(1, B_ONE), (2, B_ONE), (3, B_ONE)} <= g2 and (4, B_ONE) not in g2,
            "empty_slab": all(int(m.H[b, 1]) == 0 for b in (1, 2, 3, 4)),
            "heavy_shared": all(int(m.H[b, B_HEAVY]) > 64 * K_UNIT_CAP for b in (1, 2, 3, 4)),
        }

    return Case("B", B_ELEMS, 0, addr, L, checks)


# C / D: item-count limits of the plan, fused and launched -------------------------------------------------
def _plan_limit_case(name, elems, cus, js, thin, med, ones, heavy, large_chunks=0, tail=None):
    """Buckets 1.. with js[i] items each in whole chunks of their own. Every chunk: thin[2] records in each
    slab of [thin[0], thin[1]), med[2] in each of [med[0], med[1]); one chunk inside each item also one
    record in each slab of [ones[0], ones[1]); the rest over `heavy`. large_chunks > 0: a large push of
    that many chunks, filled up with uniform records of the other buckets. tail: records appended last."""
    small = large_chunks == 0
    item = K_STPB * K_SPER
    kchunk = K_ATPB * (K_APER if small else K_APER_PLAIN)
    n_special = sum(js) * item
    n = n_special + (0 if tail is None else tail.size) if small else large_chunks * kchunk
    L = layout(elems, n, cus, 0)
    rng = _rng(name)
    chunks = []
    for i, ji in enumerate(js):
        assert ji * item % kchunk == 0
        for k in range(ji * item // kchunk):
            counts = {f: thin[2] for f in range(thin[0], thin[1])}
            counts.update({f: med[2] for f in range(med[0], med[1])})
            if k % 3 == 0 if small else k % 3 != 1:  # once per item
                counts.update({f: 1 for f in range(ones[0], ones[1])})
            chunks.append(_chunk(rng, L, 1 + i, counts, heavy, kchunk))
    if not small:
        others = list(range(len(js) + 2, min(L["nb"], (elems >> K_SLAB_BITS) >> L["fb"])))
        chunks.append(_uniform_over(rng, L, others, n - n_special - (0 if tail is None else tail.size), elems))
    if tail is not None:
        chunks.append(tail)
    addr = np.concatenate(chunks)
    assert addr.size == n
    return L, addr


C_ELEMS = 1 << 26
C_JS = (32, 33, 63, 64)


def case_c(cus):
    """A small push (the plan fused into bin_fsort), nf = 256: nl = 257, jt = 63, kPTab holds J <= 32.
    Chunks of 4096 = item / 3, so every count per item is exact."""
    L, addr = _plan_limit_case("C", C_ELEMS, cus, C_JS, thin=(8, 72, 4), med=(128, 136, 64), ones=(208, 224),
                               heavy=[0, 1])

    def checks(m):
        b = {j: 1 + i for i, j in enumerate(C_JS)}
        g16, g4 = grouped(m, 16), grouped(m, 4)
        shared = shared_slab(m)
        return {
            "fused_nf256": bool(L["small_push"]) and L["nf"] == 256 and L["kchunk"] == 4096 and m.jt == 63,
            "items": [int(m.J[b[j]]) for j in C_JS] == list(C_JS),
            "wave_emit_to_32": wave_emit(m) == {b[32]} and walk_buckets(m) == {b[33], b[63], b[64]},
            "multitile_above_63": walk_multitile(m) == {b[64]},
            "group16": {(x, 208) for x in b.values()} <= g16,
            "group4_wave_and_walk": {(b[32], 8), (b[33], 8)} <= g4 and (b[63], 8) not in g4,
            "singles_list": {(b[63], 8), (b[64], 71)} <= sparse_list(m) | sparse_to_sweep(m),
            "medium_shared": {(x, 128) for x in b.values()} <= shared,
            "heavy_shared": {(x, 0) for x in b.values()} <= shared,
            "all_exact": bool((m.lo == m.hi).all()),
        }

    return Case("C", C_ELEMS, 0, addr, L, checks)


D_ELEMS = (1 << 28) + 4097
D_JS_SMALL = (8, 9, 15, 16, 20)
D_JS_LARGE = (32, 34, 62, 64)  # (even: whole chunks of 8192 = 2/3 item)
D_LARGE_CHUNKS = 1664


def _d_tail():
    """the shard's last slab holds one element, the last: records on it and on the slab before"""
    last = D_ELEMS - 1
    return np.array([last, last - 1, last - 4096, last, last - 1, last - 2, last], np.int64)


def case_d_small(cus):
    """nf = 1024 with the plan fused: nl = 1025, jt = 15, the wave emit holds up to J = 8. An odd count,
    the last slab partial."""
    L, addr = _plan_limit_case("Ds", D_ELEMS, cus, D_JS_SMALL, thin=(64, 576, 2), med=(600, 608, 64),
                               ones=(1008, 1024), heavy=[0, 1, 700], tail=_d_tail())

    def checks(m):
        b = {j: 1 + i for i, j in enumerate(D_JS_SMALL)}
        lb = (D_ELEMS - 1) >> (K_SLAB_BITS + L["fb"])
        return {
            "fused_nf1024": bool(L["small_push"]) and L["nf"] == 1024 and m.jt == 15 and L["kchunk"] == 4096,
            "odd_count": addr.size % 2 == 1,
            "items": [int(m.J[b[j]]) for j in D_JS_SMALL] == list(D_JS_SMALL),
            "wave_emit_to_8": wave_emit(m) - {lb} == {b[8]} and {b[9], b[15], b[16], b[20]} <= walk_buckets(m),
            "multitile_above_15": walk_multitile(m) == {b[16], b[20]},
            "group16_both_halves": all({(x, 64), (x, 560), (x, 1008)} <= grouped(m, 16) for x in b.values()),
            "shared_both_halves": all({(x, 0), (x, 700)} <= shared_slab(m) for x in b.values()),
            "last_element": int(m.addr.max()) == D_ELEMS - 1 and int(m.H[lb, 1]) == 3 and int(m.H[lb, 0]) == 4,
            "last_slab_grouped": (lb, 0) in grouped(m, 16),
        }

    return Case("D_small", D_ELEMS, 0, addr, L, checks)


def case_d_large(cus):
    """nf = 1024 in the plan launch: two planning workgroups of 512 slabs per bucket (nl = 513, jt = 63,
    the wave emit up to J = 32), both of which must emit units."""
    L, addr = _plan_limit_case("Dl", D_ELEMS, cus, D_JS_LARGE, thin=(64, 576, 4), med=(600, 608, 128),
                               ones=(1008, 1024), heavy=[0, 1, 700], large_chunks=D_LARGE_CHUNKS, tail=_d_tail())

    def checks(m):
        b = {j: 1 + i for i, j in enumerate(D_JS_LARGE)}
        ranges, _, _ = plan_shape(L)
        return {
            "launched_nf1024": not L["small_push"] and L["nf"] == 1024 and L["kchunk"] == 8192,
            "two_workgroups_of_512": ranges == [(0, 512), (512, 1024)] and m.jt == 63,
            "items": [int(m.J[b[j]]) for j in D_JS_LARGE] == list(D_JS_LARGE),
            "wave_emit_to_32": {b[32]} <= wave_emit(m) and {b[34], b[62], b[64]} <= walk_buckets(m),
            "multitile_above_63": walk_multitile(m) == {b[64]},
            "both_workgroups_emit": all(int(m.H[x, lo:hi].sum()) > 0 for x in b.values() for lo, hi in ranges),
            "ones_exact": all(m.exact(x, 1008, 16) for x in b.values()),
            "group16_both_halves": all({(x, 1008)} <= grouped(m, 16) for x in b.values()) and
            all((x, 64) in grouped(m, 4) | grouped(m, 8) | grouped(m, 16) for x in (b[32], b[34])),
            "shared_both_halves": all(int(m.H[x, f]) > K_UNIT_CAP for x in b.values() for f in (0, 700)),
            "last_element": int(m.addr.max()) == D_ELEMS - 1,
        }

    return Case("D_large", D_ELEMS, 0, addr, L, checks)


# E. bin_apply2's write-back variants at their thresholds -----------------------------------------------------
E_ROWS, E_COLS = 65537, 129
E_PITCH = E_COLS + 1
E_ELEMS = E_ROWS * E_PITCH


def _e_elements(rng, L, b, f, distinct, width=K_SLAB):
    """`distinct` elements of the slab that a matrix of E_COLS columns at pitch E_PITCH can address"""
    base = _slab_base(L, b, f)
    e = base + np.arange(width)
    e = e[e % E_PITCH != E_COLS]
    return rng.permutation(e)[:distinct]


def _e_records(rng, L, b, f, records, distinct, width=K_SLAB):
    e = _e_elements(rng, L, b, f, distinct, width)
    return np.concatenate((e, e[rng.integers(0, distinct, records - distinct)]))


def case_e(cus, unique=False, mat=False):
    """Slabs at bin_apply2's thresholds, each bucket a single item (the wave emit). unique: every element at
    most once per push (Float sums are then exact); the slabs that need duplicates change to their nearest
    shape without. mat: the model of the same addresses in a matrix shard, where slabs are not grouped."""
    rng = _rng("E")
    L = layout(E_ELEMS, 16000, cus, 0)  # (the geometry does not depend on n for a small push)
    R = lambda b, f, rec, dis=None, width=K_SLAB: _e_records(rng, L, b, f, rec, rec if dis is None or unique else dis, width)
    last_slab = (E_ELEMS - 1) >> K_SLAB_BITS
    lb, lf = last_slab >> L["fb"], last_slab & (L["nf"] - 1)
    last_width = E_ELEMS - (last_slab << K_SLAB_BITS)
    one = (768 if unique else 2048, 1)
    parts = [
        # bucket 1: lone slabs beside busy neighbours
        R(1, 0, 1100), R(1, 1, 768 if unique else 1024, 768), R(1, 2, 769 if unique else 1024, 769), R(1, 3, 1100),
        R(1, 4, 1025), R(1, 5, 1100),
        # ... an aligned group of 4 slabs with exactly 2048 distinct elements, its neighbour busy
        R(1, 8, 512), R(1, 9, 512), R(1, 10, 512), R(1, 11, 512), R(1, 12, 1100),
        # bucket 2: the same four slabs with 2049 records (a lone slab of 513, a lone one of 512, a 2-group of
        # exactly 1024), and 16 slabs with 2048 records on one element
        R(2, 0, 513), R(2, 1, 512), R(2, 2, 512), R(2, 3, 512), R(2, 20, *one),
        # the shard's last slab, partial: the leader of a group
        R(lb, lf, 60 if unique else 100, 60, last_width),
    ]
    addr = rng.permutation(np.concatenate(parts))
    L = layout(E_ELEMS, addr.size, cus, 0)

    def checks(m):
        lst, swp, dns = sparse_list(m), sparse_to_sweep(m), dense_sweep(m)
        out = {
            "small_single_items": bool(L["small_push"]) and L["nf"] == 64 and all(int(m.J[b]) == 1 for b in (1, 2, lb)),
            "matrix_addressable": bool((m.addr % E_PITCH != E_COLS).all()) and int(m.addr.max()) < E_ELEMS,
            "list_768": (1, 1) in lst and int(m.distinct[1, 1]) == K_LIST_MAX,
            "list_to_sweep_769": (1, 2) in swp and int(m.distinct[1, 2]) == K_LIST_MAX + 1,
            "dense_1025": (1, 4) in dns and int(m.H[1, 4]) == K_SPARSE_MAX2 + 1,
            "busy_neighbours_alone": {(1, 0), (1, 3), (1, 5)} <= dns,
            "last_slab_partial": last_width < K_SLAB and int(m.H[lb, lf]) > 0,
        }
        if not unique:
            out["sparse_max_1024"] = int(m.H[1, 1]) == K_SPARSE_MAX2 == int(m.H[1, 2])
        if mat:
            out["no_groups"] = bool((m.span == 1).all())
            out["singles"] = {(1, 8), (2, 0), (2, 3), (lb, lf)} <= lst
        else:
            out.update({
                "group4_full_table": (1, 8) in grouped(m, 4) and int(m.distinct[1, 8:12].sum()) == K_GROUP_CAP,
                "not_group4_at_2049": int(m.H[2, 0:4].sum()) == K_GROUP_CAP + 1 and int(m.span[2, 0]) == 1 and
                int(m.span[2, 1]) == 1,
                "group2_exactly_1024": (2, 2) in grouped(m, 2) and int(m.H[2, 2:4].sum()) == 1024,
                "group16": (2, 16) in grouped(m, 16),
                "last_slab_grouped": int(m.span[lb, lf & ~15]) == 16 and lf & 15 == 0,
            })
            if not unique:
                out["group16_one_element"] = int(m.H[2, 16:32].sum()) == K_GROUP_CAP and int(m.distinct[2, 20]) == 1
        return out

    name = "E" + ("_unique" if unique else "") + ("_mat" if mat else "")
    return Case(name, E_ELEMS, 0, addr, L, checks, cols=E_COLS if mat else 0)


CASES = {
    "A_prep": lambda cus: case_a(cus, 0),
    "A_hot": lambda cus: case_a(cus, 1),
    "B": case_b,
    "C": case_c,
    "D_small": case_d_small,
    "D_large": case_d_large,
    "E": case_e,
    "E_mat": lambda cus: case_e(cus, mat=True),
    "E_unique": lambda cus: case_e(cus, unique=True),
    "E_unique_mat": lambda cus: case_e(cus, unique=True, mat=True),
}
# The CU counts at which a case reaches its branches. Case C's 192 items are a small push (the fused plan)
# only from 65 CUs on: 64 buckets + 192 items + 1 <= 4 cus.
SUPPORTED_CUS = {name: {64, 256, 304} for name in CASES}
SUPPORTED_CUS["C"] = {256, 304}


def shape(name):
    """(elems, records, front end) of the case: what, with the CU count, its layout depends on"""
    if name not in _shapes:
        c = build(name, 256)
        _shapes[name] = (c.elems, c.n, c.front)
    return _shapes[name]


_SIG = ("small_push", "per", "kchunk", "nchunks_max", "item", "fb", "nb", "nf")
_cache = {}
_shapes = {}


def build(name, cus):
    """The case for a device of `cus` compute units, with its model as `.m` (the last few kept: a case
    and its model depend on the CU count only through the words of _SIG)."""
    for (nm, sig), c in _cache.items():
        if nm == name:
            L = layout(c.elems, c.n, cus, c.front)
            if tuple(L[k] for k in _SIG) == sig:
                if L == c.L:
                    return c
                other = Case(c.name, c.elems, c.front, c.addr, L, c.checks, c.cols)
                other.m = c.m
                return other
    c = CASES[name](cus)
    c.m = model(c.addr, c.L, group_on=not c.cols)
    while len(_cache) >= 3:
        _cache.pop(next(iter(_cache)))
    _cache[(name, tuple(c.L[k] for k in _SIG))] = c
    return c


NP_DTYPE = {"long": np.int64, "int": np.int32, "double": np.float64, "float": np.float32}


def values(case, dtype):
    """The case's record values: integers over +-2^40 (Int: +-2^30, sums wrap as the shard's do), so that a
    misplaced record cannot cancel; Double / Float uniform in [-1, 1)."""
    rng = _rng(f"{case.name}/{dtype}")
    if dtype in ("long", "int"):
        lim = 1 << 40 if dtype == "long" else 1 << 30
        return rng.integers(-lim, lim, case.n).astype(NP_DTYPE[dtype])
    return rng.uniform(-1, 1, case.n).astype(NP_DTYPE[dtype])


def keys(case):
    """(keys,) of a vector shard of case.elems elements from key 0, or (rows, cols) of the matrix shard"""
    if case.cols:
        return case.addr // (case.cols + 1), (case.addr % (case.cols + 1)).astype(np.int32)
    return (case.addr,)
