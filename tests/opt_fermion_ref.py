"""NumPy restatement of what the device-resident optimizer adds for fermionic states (peps_amd/csrc/engine_opt.h): the projection
Pi = E mask E^T on vectors in the extended layout [rows][cols][4 d][D^4], E the decoration T''[s + d var] = sigma_var * T[s] of
peps_amd/fermion.py.  Per (site, s, element): t = allowed * sum_var sigma_var x[s + d var], summed in the order var = 0, 1, 2, 3, then
x[s + d var] <- sigma_var t.  Entries past a leg's dimension (padding) come out zero."""
import numpy as np

NVAR = 4


def signs(state, r, c, s):
    """(four sign arrays, allowed mask) of stored state s at site (r, c), shape of the site tensor"""
    pl, pd, pr, pu = state.par[r][c]
    l = pl[:, None, None, None]; dd = pd[None, :, None, None]; rr = pr[None, None, :, None]; u = pu[None, None, None, :]
    shp = (len(pl), len(pd), len(pr), len(pu))
    n = int(state.nf[s])
    base = (u * n + u + dd * rr + l + l * u) % 2
    sg = (np.ones(shp), 1.0 - 2 * (u % 2) + np.zeros(shp), 1.0 - 2 * base + np.zeros(shp), 1.0 - 2 * ((base + l) % 2) + np.zeros(shp))
    return sg, ((l + dd + rr + u + n) % 2 == 0) + np.zeros(shp, dtype=bool)


def project(state, x_ext):
    d = state.d
    out = np.zeros_like(x_ext)
    for r in range(state.rows):
        for c in range(state.cols):
            for s in range(d):
                sg, allowed = signs(state, r, c, s)
                sl = tuple(slice(0, k) for k in allowed.shape)
                t = np.zeros(allowed.shape, dtype=x_ext.dtype)
                for var in range(NVAR):
                    t = t + sg[var] * x_ext[(r, c, s + d * var) + sl]
                t = t * allowed
                for var in range(NVAR):
                    out[(r, c, s + d * var) + sl] = sg[var] * t
    return out


def decorate(state, stored):
    """E: stored components [rows][cols][d][D^4] -> extended layout [rows][cols][4 d][D^4] (no parity check: any array)"""
    d = state.d
    out = np.zeros(stored.shape[:2] + (NVAR * d,) + stored.shape[3:], dtype=stored.dtype)
    for r in range(state.rows):
        for c in range(state.cols):
            for s in range(d):
                sg, _ = signs(state, r, c, s)
                sl = tuple(slice(0, k) for k in sg[0].shape)
                for var in range(NVAR):
                    out[(r, c, s + d * var) + sl] = sg[var] * stored[(r, c, s) + sl]
    return out


def stored_flat(state, D=None):
    """the stored components as one padded array [rows][cols][d][D^4]"""
    D = D or state.D
    out = np.zeros((state.rows, state.cols, state.d, D, D, D, D), dtype=np.complex128 if state.is_complex else np.float64)
    for r in range(state.rows):
        for c in range(state.cols):
            for s in range(state.d):
                a = state.tensors[r][c][s]
                out[(r, c, s) + tuple(slice(0, k) for k in a.shape)] = a
    return out


def allowed_flat(state, D=None):
    """True on the parameters of the state (parity-allowed entries inside the leg dimensions), layout of stored_flat"""
    D = D or state.D
    out = np.zeros((state.rows, state.cols, state.d, D, D, D, D), dtype=bool)
    for r in range(state.rows):
        for c in range(state.cols):
            for s in range(state.d):
                _, allowed = signs(state, r, c, s)
                out[(r, c, s) + tuple(slice(0, k) for k in allowed.shape)] = allowed
    return out
