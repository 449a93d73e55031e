"""LPScenarios: ONE constraint matrix, many right-hand sides and costs (lpx_scenarios, include/lpx.h).  The matrix goes to
the device once; every solve() sends b and c as dense arrays and runs LPSolver.solve for every scenario in ONE launch,
one workgroup per scenario, phase 1 included."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import raise_for_status


def scenario_arrays(m, n, b, c):
    """(count, b, ldb, c, ldc) as lpx_scenarios_solve takes them: b of shape (m,) or (count, m), c of shape (n,) or
    (count, n); a 1-D array is ONE vector for every scenario (pitch 0); two 2-D arrays must agree on count, two 1-D
    arrays are one scenario.  Pure numpy: no library call."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if b.ndim not in (1, 2) or b.shape[-1] != m:
        raise ValueError("b has shape %s, expected (%d,) or (count, %d)" % (b.shape, m, m))
    if c.ndim not in (1, 2) or c.shape[-1] != n:
        raise ValueError("c has shape %s, expected (%d,) or (count, %d)" % (c.shape, n, n))
    counts = {a.shape[0] for a in (b, c) if a.ndim == 2}
    if len(counts) > 1:
        raise ValueError("b has %d scenarios and c has %d" % (b.shape[0], c.shape[0]))
    count = counts.pop() if counts else 1
    return count, b, (m if b.ndim == 2 else 0), c, (n if c.ndim == 2 else 0)


class LPScenarios:
    def __init__(self, A, device=0, options=None, pricing="reference"):
        """`A`: the m x n matrix every scenario shares.  options: {"fused": 0 | 1 | 2} (the only option); without it the
        handle follows set_default_arithmetic the way LPBatch does."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2:
            raise ValueError("A is a matrix")
        L = _lib.lib()
        self._L = L
        self._h = None
        self.m, self.n = A.shape
        h = C.c_void_p()
        rc = L.lpx_scenarios_create(self.m, self.n, A.ctypes.data_as(_lib.dp) if A.size else None, max(self.n, 1),
                                    int(device), C.byref(h))
        if rc:
            raise_for_status(rc)
        self._h = h
        if _lib.PRICING[pricing]:
            rc = L.lpx_scenarios_set_pricing(h, _lib.PRICING[pricing])
            if rc:
                raise_for_status(rc)
        if _lib.DEFAULT_FUSED is not None and "fused" not in (options or {}):
            self.set_option("fused", int(_lib.DEFAULT_FUSED))
        for key, value in (options or {}).items():
            self.set_option(key, value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpx_scenarios_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        rc = self._L.lpx_scenarios_set_option(self._h, _lib.OPTIONS[key] if isinstance(key, str) else int(key), int(value))
        if rc:
            raise_for_status(rc)

    def solve(self, b, c, maximize=None, max_pivots=-1, restore_order=None):
        """LPSolver.solve for every scenario (b_k, c_k) in ONE launch.  b: (m,) or (count, m); c: (n,) or (count, n).
        maximize: one flag per scenario (None: every scenario maximises).  restore_order: None (the default-name order) or
        the ONE order of restoreInitialLP as original-variable indices (at most n; an empty one substitutes nothing).
        Returns a list of SolveInfo; .perm and .x are filled when the scenario's final state is m x n and None when its
        solve ended inside phase 1."""
        return self._solve(False, b, c, maximize, max_pivots, restore_order)

    def set_basis(self, ids):
        """The basis every later resolve() starts from (lpx_scenarios_set_basis): the m variable ids that are to be basic,
        in perm's numbering (0..n-1 the original variables, n..n+m-1 the slacks) -- the perm[n:] of a solved base case
        will do -- or None to clear it.  Returns the pivots it took to bring the matrix there (0 for None).  A singular
        basis raises and leaves the handle without one.  solve() never looks at the basis."""
        m, n = self.m, self.n
        arr = None
        if ids is not None:
            arr = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
            if arr.size != m:
                raise ValueError("a basis has %d entries, got %d" % (m, arr.size))
            if not arr.size:
                arr = np.zeros(1, dtype=np.int32)   # m = 0: the empty basis, non-NULL
        took = C.c_int32(0)
        rc = self._L.lpx_scenarios_set_basis(self._h, None if arr is None else arr.ctypes.data_as(_lib.ip), C.byref(took))
        if rc:
            raise_for_status(rc)
        return took.value

    def resolve(self, b, c, maximize=None, max_pivots=-1, restore_order=None):
        """solve() from the basis of set_basis (lpx_scenarios_resolve): every scenario's (b, c) is brought to the basis on
        chip and then takes the primal loop (b' >= 0), a dual simplex loop followed by the primal one (some b' < 0, no
        improving cost) or, where neither holds, exactly what solve() does.  Returns the SolveInfo list of solve(), each
        entry with .route in {"cold", "primal", "dual"}; on the primal and dual routes pivots_phase1 counts the dual
        loop, pivots_phase2 the primal loop, phase1_used is False and perm and x are always filled."""
        return self._solve(True, b, c, maximize, max_pivots, restore_order)

    def _solve(self, from_basis, b, c, maximize, max_pivots, restore_order):
        from .lp_solver import SolveInfo
        m, n = self.m, self.n
        cnt, b, ldb, c, ldc = scenario_arrays(m, n, b, c)
        mx = None
        if maximize is not None:
            mx = np.ascontiguousarray(np.asarray([1 if f else 0 for f in maximize], dtype=np.int32))
            if mx.shape != (cnt,):
                raise ValueError("maximize needs one flag per scenario")
        order, olen = None, -1
        if restore_order is not None:
            o = np.asarray(restore_order, dtype=np.int32).reshape(-1)
            if o.size > n:
                raise ValueError("the restore order has %d entries for %d variables" % (o.size, n))
            olen = int(o.size)
            order = np.ascontiguousarray(o) if o.size else np.zeros(1, dtype=np.int32)   # empty: non-NULL, length 0
        res = (_lib.SolveResult * max(cnt, 1))()
        x = np.full((cnt, n), -1.0)
        perm = np.full((cnt, n + m), -1, dtype=np.int32)   # -1 stays where the final state is not m x n
        args = [self._h, cnt, b.ctypes.data_as(_lib.dp) if m else None, ldb, c.ctypes.data_as(_lib.dp) if n else None, ldc,
                None if mx is None else mx.ctypes.data_as(_lib.ip), int(max_pivots),
                None if order is None else order.ctypes.data_as(_lib.ip), olen, res,
                x.ctypes.data_as(_lib.dp) if x.size else None, perm.ctypes.data_as(_lib.ip) if perm.size else None]
        if from_basis:
            route = np.zeros(max(cnt, 1), dtype=np.int32)
            rc = self._L.lpx_scenarios_resolve(*args, route.ctypes.data_as(_lib.ip))
        else:
            rc = self._L.lpx_scenarios_solve(*args)
        if rc:
            raise_for_status(rc)
        infos = [SolveInfo.of_batch_row(res[k], m, n, perm[k], x[k]) for k in range(cnt)]
        if from_basis:
            for k, info in enumerate(infos):
                info.route = _lib.ROUTES[route[k]]
        return infos
