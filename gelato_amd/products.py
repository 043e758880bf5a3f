"""ConstraintOperator: the whole constraint Jacobian of a resident batch as a pair of products.

Rows [defect 11N | K's R]: the four defect groups (Engine.jac_matvec_device / jac_rmatvec_device from the compact values) followed
by every other row (Engine.con_matvec_device / con_rmatvec_device: the row table's linear and node-function rows, the aero
kinds).  The batch is evaluated ONCE, on the device, and everything the products read stays there; no matrix is formed.
torch provides the device buffers; it is imported when an operator is built, not with the package."""
import numpy as np

from .engine import Engine, _f64


class ConstraintOperator:
    """A(x_b) for b = 0 .. B - 1 of one engine at the decision vectors X [B, nvars] (or [nvars]).

    res [B, 11N], con [B, R]: the constraint values of the evaluation (host arrays); status: its status.
    row_slices: {"mass", "pos", "vel", "quat", "linear", "nodefn", "alpha", "q", "qalpha"} -> slice of the rows."""

    def __init__(self, engine, X):
        import torch
        E = self.engine = engine
        X = _f64(X).reshape(-1, E.nvars)
        B = self.B = X.shape[0]
        d = self.dims = E.con_products_dims()
        if d["R"] == 0:
            raise ValueError("ConstraintOperator: the engine has no row table and no aero kind configured")
        self.R, self.shape = d["R"], (E.nres + d["R"], E.nvars)
        N = E.N
        o = np.cumsum([0, N, 3 * N, 3 * N, 4 * N, d["nlin"], d["nfn"], d["alpha"], d["q"], d["qalpha"]])
        self.row_slices = {k: slice(int(o[i]), int(o[i + 1]))
                           for i, k in enumerate(("mass", "pos", "vel", "quat", "linear", "nodefn") + tuple(E.AERO_KINDS))}

        def buf(*shape):
            return torch.empty(shape, dtype=torch.float64, device="cuda")
        self._torch = torch
        dx = torch.from_numpy(X).cuda()
        self._res, self._jvar = buf(B, E.nres), buf(B, max(E.V, 1))
        E.eval_batch_device(B, dx.data_ptr(), self._res.data_ptr(), self._jvar.data_ptr())
        self._con = buf(B, d["R"])
        self._jfn = buf(B, d["nfn"], 7) if d["nfn"] else None
        if d["nlin"] + d["nfn"]:
            rows = buf(B, d["nlin"] + d["nfn"])
            E.rows_eval_device(B, dx.data_ptr(), rows.data_ptr(), self._jfn.data_ptr() if d["nfn"] else 0)
            self._con[:, :d["nlin"] + d["nfn"]] = rows
        self._jac = None
        if d["alpha"] + d["q"] + d["qalpha"]:
            cons = [buf(B, d[k]) if d[k] else None for k in E.AERO_KINDS]
            self._jac = [buf(B, sum(E.aero_dims(k)[1])) if d[k] else None for k in E.AERO_KINDS]
            E.eval_aero_all_device(B, dx.data_ptr(), [c.data_ptr() if c is not None else 0 for c in cons],
                                   [j.data_ptr() if j is not None else 0 for j in self._jac])
            for k, c in zip(E.AERO_KINDS, cons):
                if c is not None:
                    self._con[:, self.row_slices[k].start - E.nres:self.row_slices[k].stop - E.nres] = c
        self.status = E.sync()
        self.res, self.con = self._res.cpu().numpy(), self._con.cpu().numpy()

    # the device pointers of vectors b0 .. of the evaluation
    def _ptrs(self, b0):
        E = self.engine
        jv = self._jvar.data_ptr() + 8 * b0 * self._jvar.shape[1]
        jfn = self._jfn.data_ptr() + 8 * b0 * self.dims["nfn"] * 7 if self._jfn is not None else 0
        jac = None
        if self._jac is not None:
            jac = [j.data_ptr() + 8 * b0 * j.shape[1] if j is not None else 0 for j in self._jac]
        return jv, jfn, jac

    def _matvec(self, V, b0, nb):
        torch, E = self._torch, self.engine
        dv = torch.from_numpy(_f64(V).reshape(nb, E.nvars)).cuda()
        y0 = torch.empty((nb, E.nres), dtype=torch.float64, device="cuda")
        y1 = torch.empty((nb, self.R), dtype=torch.float64, device="cuda")
        jv, jfn, jac = self._ptrs(b0)
        E.jac_matvec_device(nb, jv, dv.data_ptr(), y0.data_ptr())
        E.con_matvec_device(nb, jfn, jac, 0, dv.data_ptr(), y1.data_ptr())
        rc = E.sync()
        return torch.cat([y0, y1], dim=1).cpu().numpy(), rc

    def _rmatvec(self, Lam, b0, nb):
        torch, E = self._torch, self.engine
        Lam = _f64(Lam).reshape(nb, self.shape[0])
        l0 = torch.from_numpy(np.ascontiguousarray(Lam[:, :E.nres])).cuda()
        l1 = torch.from_numpy(np.ascontiguousarray(Lam[:, E.nres:])).cuda()
        g = torch.empty((nb, E.nvars), dtype=torch.float64, device="cuda")
        jv, jfn, jac = self._ptrs(b0)
        E.jac_rmatvec_device(nb, jv, l0.data_ptr(), g.data_ptr())                       # J^T lambda_defect
        E.con_rmatvec_device(nb, jfn, jac, 0, l1.data_ptr(), g.data_ptr(), accumulate=True)   # + K^T lambda_other
        rc = E.sync()
        return g.cpu().numpy(), rc

    def matvec(self, V):
        """V [B, nvars] -> y [B, 11N + R] = A(x_b) v_b (status in self.last_status)"""
        y, self.last_status = self._matvec(V, 0, self.B)
        return y

    def rmatvec(self, Lam):
        """Lam [B, 11N + R] -> g [B, nvars] = A(x_b)^T lambda_b: gel_jac_rmatvec_device, then the accumulate call of
        gel_con_rmatvec_device into the same buffer"""
        g, self.last_status = self._rmatvec(Lam, 0, self.B)
        return g

    def for_vector(self, b):
        """scipy.sparse.linalg.LinearOperator of shape (11N + R, nvars) for vector b of the batch, as Engine.jac_operator gives
        for the defect rows (scipy is imported here, not with the package)"""
        from scipy.sparse.linalg import LinearOperator
        b = int(b)
        if not 0 <= b < self.B:
            raise IndexError("vector %d of a batch of %d" % (b, self.B))
        return LinearOperator(self.shape, matvec=lambda v: self._matvec(np.asarray(v, dtype=np.float64).reshape(-1), b, 1)[0][0],
                              rmatvec=lambda lam: self._rmatvec(np.asarray(lam, dtype=np.float64).reshape(-1), b, 1)[0][0],
                              dtype=np.float64)


__all__ = ["ConstraintOperator", "Engine"]
