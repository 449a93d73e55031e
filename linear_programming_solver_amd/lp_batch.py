"""LPBatch: many small LPStates behind one handle (lpx_batch, include/lpx.h).  The device solves every LP of the batch
in ONE launch, one workgroup per LP with the LP's state in LDS; shapes may differ inside a batch."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import raise_for_status


def pack_lps(lps):
    """The arrays lpx_batch_create reads, from a list of (A, b, c) or (A, b, c, v) with A of shape m_k x n_k.
    Returns a dict: count, m_max, n_max, m[count], n[count] (int32), A[count, m_max, lda] with lda = max(n_max, 1)
    (LP k's rows at A[k, :m_k, :n_k], i.e. strideA = m_max * lda), b[count, m_max], c[count, n_max], v[count]; unused
    entries are 0.  Pure numpy: no library call."""
    items = []
    for lp in lps:
        if len(lp) not in (3, 4):
            raise ValueError("an LP of a batch is (A, b, c) or (A, b, c, v)")
        b = np.asarray(lp[1], dtype=np.float64).reshape(-1)
        c = np.asarray(lp[2], dtype=np.float64).reshape(-1)
        A = np.asarray(lp[0], dtype=np.float64)
        if A.size != b.size * c.size:
            raise ValueError("LP %d: A has %d entries, expected m*n = %d*%d" % (len(items), A.size, b.size, c.size))
        items.append((A.reshape(b.size, c.size), b, c, float(lp[3]) if len(lp) == 4 else 0.0))
    count = len(items)
    m = np.array([it[1].size for it in items], dtype=np.int32)
    n = np.array([it[2].size for it in items], dtype=np.int32)
    m_max = int(m.max()) if count else 0
    n_max = int(n.max()) if count else 0
    lda = max(n_max, 1)
    A = np.zeros((count, m_max, lda))
    b = np.zeros((count, m_max))
    c = np.zeros((count, n_max))
    v = np.zeros(count)
    for k, (Ak, bk, ck, vk) in enumerate(items):
        A[k, :m[k], :n[k]] = Ak
        b[k, :m[k]] = bk
        c[k, :n[k]] = ck
        v[k] = vk
    return {"count": count, "m_max": m_max, "n_max": n_max, "lda": lda, "strideA": m_max * lda, "m": m, "n": n,
            "A": A, "b": b, "c": c, "v": v}


def _dp(a):
    return a.ctypes.data_as(_lib.dp) if a.size else None


def _ip(a):
    return a.ctypes.data_as(_lib.ip) if a.size else None


def solve_packed(p, maximize, opts, with_solutions):
    """One of the one-shot calls on the arrays `p` of pack_lps (at least one LP), `maximize` int32 per LP and a
    SolveOptions: lpx_solve_batch, or with_solutions lpx_solve_batch_all (phase 1 in the kernel too, x and perm out).
    Returns (results, x, perm, forms the batch kernel took); x[count, n_max] and perm[count, n_max + m_max] are None
    without with_solutions, and a perm row stays -1 where the library wrote nothing: the final state is not m x n."""
    L = _lib.lib()
    cnt = p["count"]
    res = (_lib.SolveResult * cnt)()
    took = C.c_int32(0)
    args = [cnt, p["m_max"], p["n_max"], _ip(p["m"]), _ip(p["n"]), _dp(p["A"]), p["lda"], p["strideA"], _dp(p["b"]),
            _dp(p["c"]), _ip(maximize), C.byref(opts), res]
    x = perm = None
    if with_solutions:
        x = np.zeros((cnt, max(p["n_max"], 1)))
        perm = np.full((cnt, max(p["n_max"] + p["m_max"], 1)), -1, dtype=np.int32)
        rc = L.lpx_solve_batch_all(*args, _dp(x), _ip(perm), C.byref(took))
    else:
        rc = L.lpx_solve_batch(*args, C.byref(took))
    if rc:
        raise_for_status(rc)
    return res, x, perm, int(took.value)


class LPBatch:
    def __init__(self, lps, device=0, options=None, pricing="reference"):
        """`lps`: list of (A, b, c[, v]).  options: {"fused": 0 | 1 | 2} (the only option of a batch); without it the
        batch follows set_default_arithmetic the way LPState does."""
        L = _lib.lib()
        self._L = L
        self._h = None
        p = pack_lps(lps)
        self.count, self.m, self.n = p["count"], p["m"], p["n"]
        h = C.c_void_p()
        rc = L.lpx_batch_create(p["count"], p["m_max"], p["n_max"], _ip(p["m"]), _ip(p["n"]), _dp(p["A"]), p["lda"],
                                p["strideA"], _dp(p["b"]), _dp(p["c"]), _dp(p["v"]), None, int(device), C.byref(h))
        if rc:
            raise_for_status(rc)
        self._h = h
        if _lib.PRICING[pricing]:
            rc = L.lpx_batch_set_pricing(h, _lib.PRICING[pricing])
            if rc:
                raise_for_status(rc)
        if _lib.DEFAULT_FUSED is not None and "fused" not in (options or {}):
            self.set_option("fused", int(_lib.DEFAULT_FUSED))
        for key, value in (options or {}).items():
            self.set_option(key, value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpx_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.count

    def set_option(self, key, value):
        rc = self._L.lpx_batch_set_option(self._h, _lib.OPTIONS[key] if isinstance(key, str) else int(key), int(value))
        if rc:
            raise_for_status(rc)

    def simplex_loop(self, max_pivots=-1, track_slots=None):
        """The loop of LPSolver.simplex for every LP, in one launch; max_pivots is each LP's budget.  Returns
        (status[count] int32, pivots_done[count] int64, tracked slots int32[count] or None).  track_slots: one slot per
        LP to follow through the pivots (-1: none for that LP)."""
        piv = np.zeros(self.count, dtype=np.int64)
        st = np.zeros(self.count, dtype=np.int32)
        tr = None
        if track_slots is not None:
            tr = np.ascontiguousarray(np.asarray(track_slots, dtype=np.int32)).copy()
            if tr.shape != (self.count,):
                raise ValueError("track_slots needs one slot per LP")
        rc = self._L.lpx_batch_simplex_loop(self._h, int(max_pivots), piv.ctypes.data_as(_lib.i64p) if self.count else None,
                                            _ip(st), None if tr is None else _ip(tr))
        if rc:
            raise_for_status(rc)
        return st, piv, tr

    def solve(self, maximize=None, max_pivots=-1, restore_orders=None):
        """LPSolver.solve for every LP of the batch in ONE launch, phase 1 included (lpx_batch_solve); the batch must be
        as created from standard forms (A, b, c).  maximize: one flag per LP (None: every LP maximises).
        restore_orders: None (the default-name order for every LP) or one entry per LP, each None or the order of
        restoreInitialLP as original-variable indices (at most n of them; an empty one substitutes nothing).  Returns a
        list of SolveInfo; .perm and .x are filled when the LP's final state is m x n and None when the solve ended
        inside phase 1 (LPBatch.read(k) then gives the auxiliary LP)."""
        from .lp_solver import SolveInfo
        cnt = self.count
        n_max = int(self.n.max()) if cnt else 0
        mx = None
        if maximize is not None:
            mx = np.ascontiguousarray(np.asarray([1 if f else 0 for f in maximize], dtype=np.int32))
            if mx.shape != (cnt,):
                raise ValueError("maximize needs one flag per LP")
        order = olen = None
        if restore_orders is not None:
            if len(restore_orders) != cnt:
                raise ValueError("restore_orders needs one entry per LP")

            def default_name_order(n):
                out = np.zeros(max(n, 1), dtype=np.int32)
                self._L.lpx_java_default_name_order(n, out.ctypes.data_as(_lib.ip))
                return out[:n]
            order = np.zeros((cnt, max(n_max, 1)), dtype=np.int32)
            olen = np.zeros(cnt, dtype=np.int32)
            for k, o in enumerate(restore_orders):
                o = default_name_order(int(self.n[k])) if o is None else np.asarray(o, dtype=np.int32).reshape(-1)
                if o.size > int(self.n[k]):
                    raise ValueError("restore order of LP %d has %d entries for %d variables" % (k, o.size, self.n[k]))
                order[k, :o.size] = o
                olen[k] = o.size
        res = (_lib.SolveResult * max(cnt, 1))()
        rc = self._L.lpx_batch_solve(self._h, None if mx is None else _ip(mx), int(max_pivots),
                                     None if order is None else order.ctypes.data_as(_lib.ip),
                                     None if olen is None else _ip(olen), res)
        if rc:
            raise_for_status(rc)
        m_max = int(self.m.max()) if cnt else 0
        x = np.zeros((cnt, max(n_max, 1)))
        perm = np.full((cnt, max(n_max + m_max, 1)), -1, dtype=np.int32)   # -1 stays where the final state is not m x n
        rc = self._L.lpx_batch_solutions(self._h, x.ctypes.data_as(_lib.dp), perm.ctypes.data_as(_lib.ip))   # one read-back
        if rc:
            raise_for_status(rc)
        return [SolveInfo.of_batch_row(res[k], int(self.m[k]), int(self.n[k]), perm[k], x[k]) for k in range(cnt)]

    def shape(self, k):
        """(m, n) of LP k now: n + 1 columns after a solve() that ended inside phase 1."""
        m, n = C.c_int32(), C.c_int32()
        rc = self._L.lpx_batch_shape(self._h, int(k), C.byref(m), C.byref(n))
        if rc:
            raise_for_status(rc)
        return m.value, n.value

    def read(self, k):
        """(A, b, c, v, perm) of LP k, like LPState.read()."""
        k = int(k)
        if not 0 <= k < self.count:
            raise IndexError("LP %d of a batch of %d" % (k, self.count))
        m, n = self.shape(k)
        A = np.zeros((m, n))
        b = np.zeros(m)
        c = np.zeros(n)
        v = C.c_double()
        perm = np.zeros(n + m, dtype=np.int32)
        rc = self._L.lpx_batch_read(self._h, k, _dp(A), max(n, 1), _dp(b), _dp(c), C.byref(v), _ip(perm))
        if rc:
            raise_for_status(rc)
        return A, b, c, v.value, perm
