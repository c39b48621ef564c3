"""Fermionic (fZ2-graded) SplitIndexTPS on the bosonic device path.

The graded contraction of a projected fermionic PEPS equals an ordinary contraction of sign-decorated site
tensors times a sign that depends on the particle number only (statement and proof obligations:
oracle/fermion.py, tests/test_oracle_fermion.py -- this module restates the construction for the product
path and never imports the oracle):

    <S|Psi>_row = sigma(N_f) * Contract( T_v[s_v] * (-1)^{u * (fermions at sites <= v, row-major)} )
    column-major order:       decoration (-1)^{u n + u + d r + l + l u + l J_v}

so a fermionic state is uploaded as a SplitIndexTPS with 4*d "extended" components per site
(extended state = s + d * variant; variants 0/1 row-major even/odd, 2/3 column-major J = 0/1) and every
fermionic sign becomes a choice of component, i.e. an entry of the configuration table the device already
indexes the shared SITPS with.  Nearest-neighbour hops along a row (column) are adjacent in the row-major
(column-major) mode order: Jordan-Wigner sign +1, only the two sites' components change, all BMPS / BTen
environments stay valid -- the reference's flow (horizontal bonds in the row pass, vertical bonds in the
column pass, psi and psi' along the same path; square_nnn_energy_solver.h:116-201,
bond_traversal_mixin.h:113-144, square_spinless_fermion.h:134-159) runs unchanged.

Physical states: 0 = occupied (odd), 1 = empty (even) (square_spinless_fermion.h:35-37).
"""
import os

import numpy as np

ROW, COL = 0, 1
NVAR = 4


def _read_qlten_z2(path, complex_data=False):
    """one fZ2 .qlten file -> (dense array, [parity vector per leg], [direction per leg]); format: SURVEY 8c.
    complex_data: QLTEN_Complex payload (interleaved complex128)"""
    with open(path, "rb") as f:
        buf = f.read()
    pos = 0

    def tok():
        nonlocal pos
        e = buf.index(b"\n", pos)
        t = buf[pos:e]
        pos = e + 1
        return t

    rank = int(tok())
    legs = []
    for _ in range(rank):
        nsec = int(tok())
        secs = []
        for _s in range(nsec):
            qn = int(tok()); tok(); deg = int(tok()); tok()
            secs.append((qn, deg))
        d = int(tok()); dim = int(tok()); tok()
        if sum(x[1] for x in secs) != dim:
            raise ValueError("corrupt index in %s" % path)
        legs.append((secs, d))
    nblocks = int(tok())
    blocks = [[int(tok()) for _ in range(rank)] for _ in range(nblocks)]
    shape = tuple(sum(s[1] for s in secs) for secs, _ in legs)
    out = np.zeros(shape, dtype=np.complex128 if complex_data else np.float64)
    item = 16 if complex_data else 8
    offs = [np.concatenate([[0], np.cumsum([s[1] for s in secs])]) for secs, _ in legs]
    for c in blocks:
        bshape = tuple(legs[k][0][c[k]][1] for k in range(rank))
        n = int(np.prod(bshape))
        data = np.frombuffer(buf, dtype="<c16" if complex_data else "<f8", count=n, offset=pos)
        pos += n * item
        out[tuple(slice(offs[k][c[k]], offs[k][c[k] + 1]) for k in range(rank))] = data.reshape(bshape)
    par = [np.concatenate([np.full(deg, qn % 2, dtype=np.int64) for qn, deg in secs]) for secs, _ in legs]
    return out, par, [d for _, d in legs]


class FermionState:
    """tensors[r][c][s] = dense array (L, D, R, U); par[r][c] = 4 parity vectors; nf[s] = fermion parity of state s"""

    def __init__(self, tensors, par, nf):
        self.tensors, self.par, self.nf = tensors, par, np.asarray(nf, dtype=np.int64)
        self.rows, self.cols, self.d = len(tensors), len(tensors[0]), len(tensors[0][0])
        for r in range(self.rows):
            for c in range(self.cols):
                pl, pd, pr, pu = self.par[r][c]
                tot = pl[:, None, None, None] + pd[None, :, None, None] + pr[None, None, :, None] + pu[None, None, None, :]
                for s in range(self.d):
                    if np.any((np.abs(self.tensors[r][c][s]) > 0) & ((tot + self.nf[s]) % 2 == 1)):
                        raise ValueError("site tensor (%d, %d, state %d) is not parity even" % (r, c, s))

    @staticmethod
    def load(directory, complex_data=False):
        """SplitIndexTPS<.., fZ2QN>::Load layout: tps_meta.txt + tps_ten{r}_{c}_{s}.qlten, rank-5 tensors (L, D, R, U, parity);
        complex_data: a SplitIndexTPS<QLTEN_Complex, fZ2QN> dump"""
        with open(os.path.join(directory, "tps_meta.txt")) as f:
            toks = f.read().split()
        rows, cols, d = int(toks[0]), int(toks[1]), int(toks[2])
        tensors, par, nf = [[None] * cols for _ in range(rows)], [[None] * cols for _ in range(rows)], [None] * d
        for r in range(rows):
            for c in range(cols):
                comp = []
                for s in range(d):
                    a, p, dirs = _read_qlten_z2(os.path.join(directory, "tps_ten%d_%d_%d.qlten" % (r, c, s)), complex_data)
                    if a.ndim != 5 or tuple(dirs) != (-1, 1, 1, -1, -1) or a.shape[4] != 1:
                        raise ValueError("expected rank-5 fermionic site tensors (L, D, R, U, parity)")
                    if par[r][c] is None:
                        par[r][c] = tuple(p[:4])
                    elif any(not np.array_equal(par[r][c][k], p[k]) for k in range(4)):
                        raise ValueError("components of one site disagree on the parity structure of a bond")
                    if nf[s] is None:
                        nf[s] = int(p[4][0])
                    comp.append(a[..., 0])
                tensors[r][c] = comp
        return FermionState(tensors, par, nf)

    @staticmethod
    def from_stored(like, stored):
        """the state with the parity structure of `like` and the stored components `stored` [rows][cols][d][D^4] (legs padded to D),
        e.g. what hostapi.fermion_optimize_exact_sum returns"""
        stored = np.asarray(stored)
        tensors = [[[np.array(stored[(r, c, s) + tuple(slice(0, k) for k in like.tensors[r][c][s].shape)]) for s in range(like.d)]
                    for c in range(like.cols)] for r in range(like.rows)]
        return FermionState(tensors, like.par, like.nf)

    @property
    def D(self):
        return max(max(t[0].shape) for row in self.tensors for t in row)

    @property
    def is_complex(self):
        return np.iscomplexobj(self.tensors[0][0][0])

    def extended_flat(self, D=None, dtype=None):
        """upload buffer [row][col][4 d][D][D][D][D] of the decorated components (legs zero padded to D); element type of the state"""
        D = D or self.D
        dtype = dtype or (np.complex128 if self.is_complex else np.float64)
        out = np.zeros((self.rows, self.cols, NVAR * self.d, D, D, D, D), dtype=dtype)
        for r in range(self.rows):
            for c in range(self.cols):
                pl, pd, pr, pu = self.par[r][c]
                l = pl[:, None, None, None]; dd = pd[None, :, None, None]; rr = pr[None, None, :, None]; u = pu[None, None, None, :]
                for s in range(self.d):
                    a = self.tensors[r][c][s]
                    n = int(self.nf[s])
                    base = (u * n + u + dd * rr + l + l * u) % 2
                    sl = (r, c, slice(None)) + tuple(slice(0, k) for k in a.shape)
                    for var, sign in enumerate((np.ones_like(a), 1 - 2 * (u % 2) + 0 * a, 1 - 2 * base + 0 * a,
                                                1 - 2 * ((base + l) % 2) + 0 * a)):
                        out[(r, c, s + self.d * var) + tuple(slice(0, k) for k in a.shape)] = a * sign
        return out

    def ext_config(self, configs, order):
        """configs [..., rows, cols] of physical states -> extended states for the given mode order"""
        cfg = np.asarray(configs)
        occ = self.nf[cfg] % 2
        shp = cfg.shape
        if order == ROW:
            flat = occ.reshape(shp[:-2] + (-1,))
            incl = np.cumsum(flat, axis=-1) % 2
            return (cfg + self.d * incl.reshape(shp)).astype(np.int32)
        flat = np.swapaxes(occ, -1, -2).reshape(shp[:-2] + (-1,))
        before = (np.cumsum(flat, axis=-1) - flat) % 2
        before = np.swapaxes(before.reshape(shp[:-2] + (shp[-1], shp[-2])), -1, -2)
        return (cfg + self.d * (2 + before)).astype(np.int32)

    def sigma(self, configs):
        nf = np.sum(self.nf[np.asarray(configs)] % 2, axis=(-1, -2))
        return 1 - 2 * ((nf + nf * (nf - 1) // 2) % 2)

    def kappa(self, configs):
        """sign of reordering the occupied modes from row-major to column-major order (per configuration)"""
        cfg = np.asarray(configs)
        occ = self.nf[cfg] % 2
        lead = cfg.shape[:-2]
        out = np.ones(lead, dtype=np.int64)
        for ix in np.ndindex(*lead):
            o = occ[ix]
            keys = [(c, r) for r in range(self.rows) for c in range(self.cols) if o[r, c]]
            inv = sum(1 for i in range(len(keys)) for j in range(i + 1, len(keys)) if keys[i] > keys[j])
            out[ix] = 1 - 2 * (inv % 2)
        return out


def fold_gradient(state, grad_ext):
    """gradient with respect to the extended (decorated) components [rows][cols][4 d][D^4] -> gradient with respect
    to the stored components [rows][cols][d][D^4]: T''[s + d var] = sign_var * T[s], so dE/dT[s] = sum_var sign_var *
    dE/dT''[s + d var]; parity-forbidden entries (not parameters of a Z2-symmetric state) are zeroed."""
    rows, cols, d = state.rows, state.cols, state.d
    D = grad_ext.shape[3]
    out = np.zeros((rows, cols, d, D, D, D, D), dtype=grad_ext.dtype)
    for r in range(rows):
        for c in range(cols):
            pl, pd, pr, pu = state.par[r][c]
            l = pl[:, None, None, None]; dd = pd[None, :, None, None]; rr = pr[None, None, :, None]; u = pu[None, None, None, :]
            shp = (len(pl), len(pd), len(pr), len(pu))
            sl = tuple(slice(0, k) for k in shp)
            for s in range(d):
                n = int(state.nf[s])
                base = (u * n + u + dd * rr + l + l * u) % 2
                allowed = ((l + dd + rr + u + n) % 2 == 0)
                signs = (np.ones(shp), 1 - 2 * (u % 2) + np.zeros(shp), 1 - 2 * base + np.zeros(shp), 1 - 2 * ((base + l) % 2) + np.zeros(shp))
                acc = np.zeros(shp, dtype=grad_ext.dtype)
                for var in range(NVAR):
                    acc += signs[var] * grad_ext[(r, c, s + d * var) + sl]
                out[(r, c, s) + sl] = acc * allowed
    return out


def evaluate_amplitude(ctx, state, configs):
    """<S|Psi> (parity legs in row-major order) for a batch of physical configurations; ctx must hold
    state.extended_flat() (phys_dim = 4 d)."""
    ctx.set_configs(state.ext_config(configs, ROW))
    return state.sigma(configs) * ctx.evaluate_amplitude()


def tj_energy(ctx, state, configs, t, J, V=0.0, mu=0.0, t2=0.0, bonds=None, nnn="slice"):
    """E_loc(S) of the t-t'-J-V model (square_tJ_model.h:301-345, :424-463 + :215-228; states 0 up, 1 down, 2 empty):
    H = -t sum_<ij> (c+ c + h.c.) - t2 sum_<<ij>> (c+ c + h.c.) + J sum (S.S - n n / 4) + V sum n n - mu N.  The diagonal hop moves an
    electron into a hole (never exchanges two spins); nnn names its path as in spinless_fermion_energy.  `bonds` (a dict) receives
    the per-bond energies "h", "v" and, with t2, "dr" / "ur"."""
    def bond(c1, c2):
        same = c1 == c2
        hole = (c1 == 2) | (c2 == 2)
        diag = np.where(same, np.where(c1 == 2, 0.0, V), np.where(hole, 0.0, -0.5 * J + V))
        off = np.where(same, 0.0, np.where(hole, -t, 0.5 * J))
        return diag, off
    e, psis = nn_energy(ctx, state, configs, bond, bonds)
    if t2 != 0.0:
        e = e + _NNN_PATHS[nnn](ctx, state, configs, t2, bonds)
    return e - mu * np.sum(np.asarray(configs) != 2, axis=(1, 2)), psis


def spinless_fermion_energy(ctx, state, configs, t, V=0.0, t2=0.0, bonds=None, nnn="local"):
    """E_loc(S) of H = -t sum_<ij> (c+_i c_j + h.c.) - t2 sum_<<ij>> (c+_i c_j + h.c.) + V sum_<ij> n_i n_j
    (square_spinless_fermion.h:134-200).  Returns (energy [n], psi_list [rows + cols][n]).  The NN hops are local
    replacements inside the row / column pass.  The diagonal hop (t2): nnn = "local" (round 5) reuses the environments of the
    row pass -- a plaquette replacement against parity-twisted BTen2 environments (nnn_hop_energy_local); nnn = "fresh" takes
    every hopped amplitude from a fresh contraction (nnn_hop_energy, rounds 2-4; kept as the independent check); nnn = "slice" is
    "local" with one device call per row pair (nnn_hop_energy_slice)."""
    nf = state.nf
    def bond(c1, c2):
        return V * (nf[c1] % 2) * (nf[c2] % 2), np.where(c1 != c2, -t, 0.0)
    e, psis = nn_energy(ctx, state, configs, bond, bonds)
    if t2 != 0.0:
        e = e + _NNN_PATHS[nnn](ctx, state, configs, t2, bonds)
    return e, psis


def nnn_hop_energy_slice(ctx, state, configs, t2, bonds=None):
    """nnn_hop_energy_local with the whole row pair in ONE device call (pepsgpu_nnn_hop_slice_fermion): the twisted chains, the
    candidates, the Jordan-Wigner signs and the closing traces stay on the device, one read-back per row pair.  A hop exists where
    the occupation state.nf differs at the two ends of a diagonal."""
    from .capi import UP, DOWN
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    dt = np.complex128 if state.is_complex else np.float64
    e = np.zeros(n, dt)
    if bonds is not None:
        bonds.update(dr=np.zeros((n, rows - 1, cols - 1), dt), ur=np.zeros((n, rows - 1, cols - 1), dt))
    if cols < 2 or rows < 2:
        return e
    nf = np.asarray(state.nf) % 2
    ctx.set_configs(state.ext_config(cfg, ROW))
    ctx.generate_bmps_approach(UP)
    for row in range(rows - 1):
        psi, val = ctx.nnn_hop_slice_fermion(row, nf, 3)
        eb = -t2 * np.conj(val / np.where(psi == 0, 1.0, psi)[:, :, None])      # (val is 0 where the hop is forbidden)
        e += eb.sum(axis=(1, 2))
        if bonds is not None:
            bonds["dr"][:, row, :] = eb[:, :, 0]
            bonds["ur"][:, row, :] = eb[:, :, 1]
        if row < rows - 2:
            ctx.shift_bmps_window(DOWN)
    return e


def nnn_hop_energy_local(ctx, state, configs, t2, bonds=None):
    """The diagonal hops of all plaquettes with the environments of ONE row pass (the reference's flow,
    square_nnn_energy_solver.h:203-265: BTen2 environments of the row pair, ReplaceNNNSiteTrace per diagonal).

    The reference's graded ReplaceNNNSiteTrace carries the signs in the tensor algebra.  In the sign-decorated form a hop between
    a = (r, c) / (r+1, c) and b = (r+1, c+1) / (r, c+1) flips the variant (parity of the fermion count up to and including the
    site, row-major) of every site between the two ends: row r right of the plaquette and row r+1 left of it.  A variant flip of
    a whole row is a second configuration table, so the hopped amplitude is a local replacement of the four plaquette tensors
    against TWISTED environments: the LEFT BTen2 grown with row r+1 flipped, the RIGHT BTen2 grown with row r flipped
    (pepsgpu_cfg_override_slice + the second BTen2 set, pepsgpu_replace_plaquette_trace).  psi of the same plaquette comes from
    the untwisted set along the same path.  Cost per row pair: two more BTen2 chains instead of 2 (cols - 1) fresh contractions."""
    from .capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    d = state.d
    occ = (np.asarray(state.nf)[cfg] % 2).reshape(n, -1)
    ext = state.ext_config(cfg, ROW)
    flip = np.where(ext // d == 0, ext + d, ext - d).astype(np.int32)       # variant 0 <-> 1 (row-major variants)
    dt = np.complex128 if state.is_complex else np.float64
    e = np.zeros(n, dt)
    if bonds is not None:
        bonds.update(dr=np.zeros((n, rows - 1, cols - 1), dt), ur=np.zeros((n, rows - 1, cols - 1), dt))
    if cols < 2 or rows < 2:
        return e
    ctx.set_configs(ext)
    ctx.generate_bmps_approach(UP)                      # DOWN stack complete, UP at the vacuum
    try:
        for row in range(rows - 1):
            # untwisted set 0 and twisted set 1: the whole RIGHT stack at once (its levels are read by index), LEFT step by step
            ctx.bten2_select_set(0)
            ctx.grow_full_bten2(RIGHT, row, 2, True)
            ctx.init_bten2(LEFT, row)
            ctx.bten2_select_set(1)
            ctx.cfg_override_slice(HORIZONTAL, row, flip[:, row, :])
            ctx.grow_full_bten2(RIGHT, row, 2, True)
            ctx.cfg_override_slice(HORIZONTAL, row + 1, flip[:, row + 1, :])
            ctx.init_bten2(LEFT, row)
            for col in range(cols - 1):
                # (the plaquette's own states are handed over explicitly: a site that reads a configuration table would read the
                # override that is set for the twisted chain)
                own = np.stack([ext[:, row, col], ext[:, row + 1, col], ext[:, row + 1, col + 1], ext[:, row, col + 1]], axis=-1)
                psi = ctx.replace_plaquette_trace(row, col, own[:, None, :], 0, 0)[:, 0]
                cands, terms = [], []
                for key, a, b in (("dr", (row, col), (row + 1, col + 1)), ("ur", (row + 1, col), (row, col + 1))):
                    differ = occ[:, a[0] * cols + a[1]] != occ[:, b[0] * cols + b[1]]      # a hop needs exactly one end occupied
                    ia, ib = sorted((a[0] * cols + a[1], b[0] * cols + b[1]))
                    jw = (-1.0) ** occ[:, ia + 1:ib].sum(axis=1)
                    new = cfg.copy()
                    new[:, a[0], a[1]], new[:, b[0], b[1]] = cfg[:, b[0], b[1]], cfg[:, a[0], a[1]]
                    ne = state.ext_config(new, ROW)
                    cands.append(np.stack([ne[:, row, col], ne[:, row + 1, col], ne[:, row + 1, col + 1], ne[:, row, col + 1]], axis=-1))
                    terms.append((key, differ, jw))
                if any(t[1].any() for t in terms):
                    psi_ex = ctx.replace_plaquette_trace(row, col, np.stack(cands, axis=1), 1, 1)
                    for k, (key, differ, jw) in enumerate(terms):
                        eb = np.where(differ, -t2 * jw * np.conj(psi_ex[:, k] / np.where(psi == 0, 1.0, psi)), 0.0)
                        e += eb
                        if bonds is not None:
                            bonds[key][:, row, col] = eb
                if col < cols - 2:          # both LEFT chains advance over column col (set 1 under the row+1 override)
                    ctx.grow_bten2_step(LEFT, row)
                    ctx.bten2_select_set(0)
                    ctx.cfg_override_slice(HORIZONTAL, row + 1, None)
                    ctx.grow_bten2_step(LEFT, row)
                    ctx.bten2_select_set(1)
                    ctx.cfg_override_slice(HORIZONTAL, row + 1, flip[:, row + 1, :])
            ctx.cfg_override_slice(HORIZONTAL, row + 1, None)
            ctx.bten2_select_set(0)
            if row < rows - 2:
                ctx.shift_bmps_window(DOWN)
    finally:
        ctx.cfg_override_slice(HORIZONTAL, 0, None)
        ctx.bten2_select_set(0)
    return e


def nnn_hop_energy(ctx, state, configs, t2, bonds=None):
    """sum over plaquette diagonals of -t2 * jw * psi(S with the two sites exchanged) / psi(S), jw = Jordan-Wigner string
    of the sites strictly between the two in row-major order (square_spinless_fermion.h:161-200): one batched fresh
    contraction per diagonal.  bonds["dr"] / ["ur"] [n, rows-1, cols-1] receive the per-bond terms."""
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    occ = (np.asarray(state.nf)[cfg] % 2).reshape(n, -1)
    psi0 = evaluate_amplitude(ctx, state, cfg)
    dt = np.complex128 if state.is_complex else np.float64
    e = np.zeros(n, dt)
    if bonds is not None:
        bonds.update(dr=np.zeros((n, rows - 1, cols - 1), dt), ur=np.zeros((n, rows - 1, cols - 1), dt))
    for row in range(rows - 1):
        for col in range(cols - 1):
            for key, a, b in (("dr", (row, col), (row + 1, col + 1)), ("ur", (row + 1, col), (row, col + 1))):
                differ = occ[:, a[0] * cols + a[1]] != occ[:, b[0] * cols + b[1]]          # a hop needs exactly one end occupied
                if not differ.any():
                    continue
                ia, ib = sorted((a[0] * cols + a[1], b[0] * cols + b[1]))
                jw = (-1.0) ** occ[:, ia + 1:ib].sum(axis=1)
                new = cfg.copy()
                new[:, a[0], a[1]], new[:, b[0], b[1]] = cfg[:, b[0], b[1]], cfg[:, a[0], a[1]]
                eb = np.where(differ, -t2 * jw * np.conj(evaluate_amplitude(ctx, state, new) / np.where(psi0 == 0, 1.0, psi0)), 0.0)
                e += eb
                if bonds is not None:
                    bonds[key][:, row, col] = eb
    return e


_NNN_PATHS = {"local": nnn_hop_energy_local, "fresh": nnn_hop_energy, "slice": nnn_hop_energy_slice}


def spinless_fermion_observables(ctx, state, configs, t, V=0.0, t2=0.0):
    """Registry of SquareNNNModelMeasurementSolver<SquareSpinlessFermion>::EvaluateObservables
    (square_nnn_model_measurement_solver.h:33-210, square_spinless_fermion.h:87-115) for a batch of configurations:
    energy [n, 1], charge [n, rows*cols] (1 - config), bond_energy_h / _v and the (t2 = 0) diagonal bonds.
    Also returns psi_list [rows + cols][n]."""
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    dt = np.complex128 if state.is_complex else np.float64
    bonds = {"dr": np.zeros((n, rows - 1, cols - 1), dt), "ur": np.zeros((n, rows - 1, cols - 1), dt)}
    e, psis = spinless_fermion_energy(ctx, state, cfg, t, V, t2, bonds)
    return {"energy": e[:, None], "charge": (1.0 - cfg).reshape(n, -1), "bond_energy_h": bonds["h"].reshape(n, -1),
            "bond_energy_v": bonds["v"].reshape(n, -1), "bond_energy_dr": bonds["dr"].reshape(n, -1),
            "bond_energy_ur": bonds["ur"].reshape(n, -1)}, psis


def tj_pair_table():
    """The configurations a pair operator connects the states (a, b) of a nearest-neighbour bond of the t-J model to (0 up, 1 down,
    2 empty), [3 * 3][2][2] over physical states, (-1, -1) for none: (empty, empty) -> (up, down), (down, up); (up, down) and
    (down, up) -> (empty, empty).  The pair table of pepsgpu_nn_pair_slice_fermion."""
    tab = -np.ones((9, 2, 2), dtype=np.int32)
    tab[2 * 3 + 2] = ((0, 1), (1, 0))
    tab[0 * 3 + 1, 0] = (2, 2)
    tab[1 * 3 + 0, 0] = (2, 2)
    return tab


def exchange_table(state, order):
    """The exchange of two sites adjacent in the mode order over pairs of extended states, [(4 d)^2][2] (the host layer's
    TPSWaveFunctionComponent::ExchangeTable): a pair whose variants do not belong to `order` maps to itself."""
    d = state.d
    dp = NVAR * d
    nf = np.asarray(state.nf) % 2
    e1, e2 = np.meshgrid(np.arange(dp), np.arange(dp), indexing="ij")
    a1, v1, a2, v2 = e1 % d, e1 // d, e2 % d, e2 // d
    na, nb = nf[a2], nf[a1]                                   # the exchanged physical states (a, b) = (a2, a1)
    if order == ROW:
        ok = (v1 < 2) & (v2 < 2)
        before = (v1 & 1) ^ nf[a1]
        c1, c2 = a2 + d * (before ^ na), a1 + d * (before ^ na ^ nb)
    else:
        ok = (v1 >= 2) & (v2 >= 2)
        before = v1 & 1
        c1, c2 = a2 + d * (2 + before), a1 + d * (2 + (before ^ na))
    return np.stack([np.where(ok, c1, e1), np.where(ok, c2, e2)], axis=-1).reshape(dp * dp, 2).astype(np.int32)


def _pair_slice_by_calls(ctx, state, cfg, orient, order, lo, hi, s, table):
    """what Context.nn_pair_slice_fermion returns, from per-bond Trace + ReplaceNNSiteTrace calls with the candidates built on the
    host from ext_config of the changed configurations"""
    from .capi import HORIZONTAL
    n = cfg.shape[0]
    N = cfg.shape[2] if orient == HORIZONTAL else cfg.shape[1]
    dt = np.complex128 if state.is_complex else np.float64
    psi, ex, pair = np.zeros((n, N - 1), dt), np.zeros((n, N - 1), dt), np.zeros((n, N - 1, 2), dt)
    ctx.init_bten(lo, s)
    ctx.grow_full_bten(hi, s, 2, True)
    for j in range(N - 1):
        (r1, c1), (r2, c2) = ((s, j), (s, j + 1)) if orient == HORIZONTAL else ((j, s), (j + 1, s))
        a, b = cfg[:, r1, c1], cfg[:, r2, c2]
        pc = table[a * state.d + b]                           # [n][2][2]
        has = pc[:, :, 0] >= 0
        cands = []
        for na, nb in [(b, a)] + [(np.where(has[:, k], pc[:, k, 0], a), np.where(has[:, k], pc[:, k, 1], b)) for k in range(2)]:
            new = cfg.copy()
            new[:, r1, c1], new[:, r2, c2] = na, nb
            ne = state.ext_config(new, order)
            cands.append(np.stack([ne[:, r1, c1], ne[:, r2, c2]], axis=-1))
        psi[:, j] = ctx.trace(r1, c1, orient)
        res = ctx.replace_nn_trace(r1, c1, orient, np.stack(cands, axis=1))
        ex[:, j] = np.where(a != b, res[:, 0], psi[:, j])
        nfs = np.asarray(state.nf) % 2
        for k in range(2):
            keeps = nfs[np.where(has[:, k], pc[:, k, 0], a)] + nfs[np.where(has[:, k], pc[:, k, 1], b)] == nfs[a] + nfs[b]
            pair[:, j, k] = np.where(has[:, k], np.where(keeps, 1.0, -1.0) * res[:, 1 + k], 0.0)      # Sigma(S') / Sigma(S)
        if j + 2 < N:
            ctx.shift_bten_window(hi)
    return psi, ex, pair


def tj_observables(ctx, state, configs, t, J, V=0.0, mu=0.0, t2=0.0, pair="slice"):
    """Registry of SquareNNNModelMeasurementSolver<SquaretJVModel>::EvaluateObservables (square_tJ_model.h:546-603, :730-850) for a batch
    of configurations, driven from Python: energy [n, 1], spin_z, charge [n, rows * cols], bond_energy_h / _v / _dr / _ur and the
    bond-singlet pairing order SC_bond_singlet_h / _v.  Also returns psi_list [rows + cols][n].

    Convention: |S> = product of c+ over the occupied sites in row-major order; Delta+_ij = (c+_i,up c+_j,down - c+_i,down c+_j,up) /
    sqrt(2) with i the left / upper site.  With rho(S') = jw psi(S') / psi(S): (empty, empty) gives delta_dag = conj(rho(up, down) -
    rho(down, up)) / sqrt(2); (up, down) gives delta = conj(rho(empty, empty)) / sqrt(2), (down, up) its negative; the registry value is
    (conj(delta_dag) + delta) / 2.  Inside a pass the two sites are adjacent modes and rho = -ReplaceNNSiteTrace / Trace: the
    decoration leaves out Sigma = (-1)^(nf (nf + 1) / 2), which a pair move flips.
    pair = "slice": one pepsgpu_nn_pair_slice_fermion per row / column; "calls": Trace + ReplaceNNSiteTrace per bond."""
    from .capi import LEFT, DOWN, RIGHT, UP, HORIZONTAL, VERTICAL
    if pair not in ("slice", "calls"):
        raise ValueError("tj_observables: pair must be 'slice' or 'calls'")
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    dt = np.complex128 if state.is_complex else np.float64
    table, nf = tj_pair_table(), np.asarray(state.nf) % 2
    out = {"h": np.zeros((n, rows, cols - 1), dt), "v": np.zeros((n, rows - 1, cols), dt),
           "sc_h": np.zeros((n, rows, cols - 1), dt), "sc_v": np.zeros((n, rows - 1, cols), dt)}
    psis = []
    isq2 = 1.0 / np.sqrt(2.0)
    for orient, order, approach, step, lo, hi, key in ((HORIZONTAL, ROW, UP, DOWN, LEFT, RIGHT, "h"), (VERTICAL, COL, LEFT, RIGHT, UP, DOWN, "v")):
        S, N = (rows, cols) if orient == HORIZONTAL else (cols, rows)
        ctx.set_configs(state.ext_config(cfg, order))
        xtab = exchange_table(state, order)
        ctx.generate_bmps_approach(approach)
        for s in range(S):
            if pair == "slice":
                psi, ex, pr = ctx.nn_pair_slice_fermion(orient, s, nf, table, xtab)
            else:
                psi, ex, pr = _pair_slice_by_calls(ctx, state, cfg, orient, order, lo, hi, s, table)
            if np.any(psi == 0):
                raise RuntimeError("Wavefunction amplitude is near zero, causing division by zero.")
            psis.append(psi[:, 0])
            for j in range(N - 1):
                (r1, c1), (r2, c2) = ((s, j), (s, j + 1)) if orient == HORIZONTAL else ((j, s), (j + 1, s))
                a, b = cfg[:, r1, c1], cfg[:, r2, c2]
                same, hole = a == b, (a == 2) | (b == 2)
                ratio = np.conj(ex[:, j] / psi[:, j])
                e = np.where(same, np.where(a == 2, 0.0, V), np.where(hole, -t * ratio, (-0.5 + 0.5 * ratio) * J + V))
                rho = pr[:, j, :] / psi[:, j, None]
                sc = np.where((a == 2) & (b == 2), (rho[:, 0] - rho[:, 1]) * isq2,
                              np.where((a == 0) & (b == 1), np.conj(rho[:, 0]) * isq2,
                                       np.where((a == 1) & (b == 0), -np.conj(rho[:, 0]) * isq2, 0.0))) / 2
                out[key][:, r1, c1], out["sc_" + key][:, r1, c1] = e, sc
            if s + 1 < S:
                ctx.shift_bmps_window(step)
    bonds = {"dr": np.zeros((n, rows - 1, cols - 1), dt), "ur": np.zeros((n, rows - 1, cols - 1), dt)}
    energy = out["h"].sum(axis=(1, 2)) + out["v"].sum(axis=(1, 2)) - mu * np.sum(cfg != 2, axis=(1, 2))
    if t2 != 0.0:
        energy = energy + nnn_hop_energy_slice(ctx, state, cfg, t2, bonds)
    return {"energy": energy[:, None], "spin_z": np.where(cfg == 0, 0.5, np.where(cfg == 1, -0.5, 0.0)).reshape(n, -1),
            "charge": (cfg != 2).astype(np.float64).reshape(n, -1), "bond_energy_h": out["h"].reshape(n, -1),
            "bond_energy_v": out["v"].reshape(n, -1), "bond_energy_dr": bonds["dr"].reshape(n, -1),
            "bond_energy_ur": bonds["ur"].reshape(n, -1), "SC_bond_singlet_h": out["sc_h"].reshape(n, -1),
            "SC_bond_singlet_v": out["sc_v"].reshape(n, -1)}, np.array(psis)


# ---- the singlet-pair correlation of the t-J models (model_solvers/base/singlet_pair_correlation_measurement_mixin.h) ----
def sc_pair_corr_ref_bonds(rows, cols, ref_bonds=()):
    """the reference bonds (y, x) measured, in output order (:193-212): all horizontal bonds of the rows above the last one, or the
    selection without its out-of-lattice members sorted by (y, x)"""
    if rows < 2 or cols < 2:
        return []
    if len(ref_bonds) == 0:
        return [(y, x) for y in range(rows - 1) for x in range(cols - 1)]
    return sorted((int(y), int(x)) for y, x in ref_bonds if 0 <= y < rows - 1 and 0 <= x < cols - 1)


def sc_pair_corr_mapping(rows, cols, ref_bonds=()):
    """GenerateSCPairCorrIndexMapping (:176-215): [(ref_y, ref_x, 0, tgt_y, tgt_x, 0)] per value of SC_singlet_pair_corr"""
    return [(y1, x1, 0, y2, x2, 0) for y1, x1 in sc_pair_corr_ref_bonds(rows, cols, ref_bonds)
            for y2 in range(y1 + 1, rows) for x2 in range(cols - 1)]


def tj_pair_inject_table():
    """(empty, empty) -> slot 0 (up, down), slot 1 (down, up): Delta+ on the reference bond"""
    tab = -np.ones((9, 2, 2), dtype=np.int32)
    tab[2 * 3 + 2] = ((0, 1), (1, 0))
    return tab


def tj_pair_remove_table():
    """(up, down), (down, up) -> slot 0 (empty, empty): Delta on the target bond"""
    tab = -np.ones((9, 2, 2), dtype=np.int32)
    tab[0 * 3 + 1, 0] = (2, 2)
    tab[1 * 3 + 0, 0] = (2, 2)
    return tab


def tj_pair_identity_table():
    """(up, down), (down, up) -> slot 0 themselves: the unreplaced two-site trace of the target bond (psi_original)"""
    tab = -np.ones((9, 2, 2), dtype=np.int32)
    tab[0 * 3 + 1, 0] = (0, 1)
    tab[1 * 3 + 0, 0] = (1, 0)
    return tab


def _pair_scan_by_calls(walker, bottom, ext_row, cfg_row, state, table):
    """what Walker.pair_trace_slice returns without a mask, from InitBTenLeft / InitBTenRight / TraceWithTwoSiteBTen /
    ShiftBTenWindow calls with the candidates built on the host; ext_row / cfg_row [n][cols] the extended / physical states of the
    MPO's row"""
    from .capi import RIGHT
    n, cols = cfg_row.shape
    d, nfs = state.d, np.asarray(state.nf) % 2
    out = np.zeros((n, cols - 1, 2), dtype=np.complex128 if state.is_complex else np.float64)
    walker.InitBTenLeft(bottom, 0)
    walker.InitBTenRight(bottom, 1)
    for x in range(cols - 1):
        a, b = cfg_row[:, x], cfg_row[:, x + 1]
        e1 = ext_row[:, x]
        before = ((e1 // d) & 1) ^ nfs[a]
        pc = table[a * d + b]                                 # [n][2][2]
        for k in range(2):
            has = pc[:, k, 0] >= 0
            if not has.any():
                continue
            pa, pb = np.where(has, pc[:, k, 0], a), np.where(has, pc[:, k, 1], b)
            c1, c2 = pa + d * (before ^ nfs[pa]), pb + d * (before ^ nfs[pa] ^ nfs[pb])
            sign = np.where(nfs[pa] + nfs[pb] == nfs[a] + nfs[b], 1.0, -1.0)
            tr = walker.TraceWithTwoSiteBTen(bottom, x, states=np.stack([c1, c2], axis=-1))
            out[:, x, k] = np.where(has, sign * tr, 0.0)
        if x < cols - 2:
            walker.ShiftBTenWindow(bottom, RIGHT)
    return out


def tj_pair_correlation(ctx, state, configs, ref_bonds=(), scan="slice"):
    """SC_singlet_pair_corr of MeasureSingletPairCorrelation (singlet_pair_correlation_measurement_mixin.h:349-534) for a batch of
    configurations, driven from Python: [n][number of bond pairs] in the order of sc_pair_corr_mapping.

    Convention (tj_observables): for the reference bond (y1, x1)-(y1, x1 + 1) and the target bond (y2, x2)-(y2, x2 + 1), y2 > y1, the
    value is non-zero only for an (empty, empty) reference and an (up, down) / (down, up) target:
        1/2 conj(rho_ud - rho_du) * (+1 for (up, down), -1 for (down, up)),  rho_x = psi(S: ref -> x, target -> (empty, empty)) / psi(S);
    its |psi|^2-weighted mean is <Delta+_ref Delta_tgt>.  Both bonds are adjacent modes of the row-major order, so each move changes the
    components of its two sites only and rho is the ratio of two-site traces of three walkers forked from up_stack[y1]: two evolved
    through the row y1 with the pair injected, one through the row itself (psi(S) along the same path; shared by the reference bonds
    of one y1).  Sigma(S') / Sigma(S) is -1 for the injection and -1 for the removal.
    scan = "slice": set_mpo_excited_pair + one pair_trace_slice per walker and target row; "calls": set_mpo_states and the per-call
    entries.  A reference bond that is (empty, empty) for no configuration of the batch creates no excited walker."""
    from .capi import DOWN, UP
    if scan not in ("slice", "calls"):
        raise ValueError("tj_pair_correlation: scan must be 'slice' or 'calls'")
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    dt = np.complex128 if state.is_complex else np.float64
    bonds = sc_pair_corr_ref_bonds(rows, cols, ref_bonds)
    mapping = sc_pair_corr_mapping(rows, cols, ref_bonds)
    out = np.zeros((n, len(mapping)), dtype=dt)
    if not bonds:
        return out
    nf = np.asarray(state.nf) % 2
    inject, remove, ident = tj_pair_inject_table(), tj_pair_remove_table(), tj_pair_identity_table()
    ext = state.ext_config(cfg, ROW)
    ctx.set_configs(ext)
    ctx.generate_bmps_approach(UP)
    ctx.grow_full_bmps(UP)
    max_ref_y = max(y for y, _ in bonds)
    if ctx.bmps_stack_size(UP) <= max_ref_y:
        raise RuntimeError("MeasureSingletPairCorrelation: UP BMPS stack insufficient.")
    if ctx.bmps_stack_size(DOWN) < rows:
        raise RuntimeError("MeasureSingletPairCorrelation: DOWN BMPS stack insufficient.")
    is_pair = ((cfg[:, :, :-1] == 0) & (cfg[:, :, 1:] == 1)) | ((cfg[:, :, :-1] == 1) & (cfg[:, :, 1:] == 0))     # [n][rows][cols - 1]
    tgt_sign = np.where(cfg[:, :, :-1] == 0, 1.0, -1.0)

    def scan_rows(walker, y1, table, mask):
        """the walker has absorbed rows [0, y1]: {y2: [n][cols - 1] slot 0 of the scan of row y2}"""
        res = {}
        for y2 in range(y1 + 1, rows):
            if y2 > y1 + 1:
                walker.set_mpo(y2 - 1)
                walker.Evolve()
            walker.set_mpo(y2)
            if scan == "slice":
                res[y2] = walker.pair_trace_slice(rows - 1 - y2, nf, table, mask)[:, :, 0]
            else:
                res[y2] = np.where(mask[:, None], _pair_scan_by_calls(walker, rows - 1 - y2, ext[:, y2, :], cfg[:, y2, :], state, table)[:, :, 0], 0.0)
            walker.ClearBTen()
        return res

    pos = 0
    psi_y1, psi_orig = -1, None
    for y1, x1 in bonds:
        npair = (rows - 1 - y1) * (cols - 1)
        ref_valid = (cfg[:, y1, x1] == 2) & (cfg[:, y1, x1 + 1] == 2)
        if not ref_valid.any():
            pos += npair
            continue
        if psi_y1 != y1:                                      # the original walker: its numbers do not depend on x1
            with ctx.get_walker(UP, level=y1) as w:
                w.set_mpo(y1)
                w.Evolve()
                psi_orig, psi_y1 = scan_rows(w, y1, ident, np.ones(n, dtype=bool)), y1
        over = []
        for k in range(2):
            with ctx.get_walker(UP, level=y1) as w:
                if scan == "slice":
                    opened, sign = w.set_mpo_excited_pair(y1, x1, nf, inject, slot=k)
                    assert np.array_equal(opened, ref_valid) and np.all(sign[ref_valid] == -1)
                else:
                    new = cfg[:, y1, :].copy()
                    new[ref_valid, x1], new[ref_valid, x1 + 1] = inject[8, k]
                    full = cfg.copy()
                    full[:, y1, :] = new
                    w.set_mpo_states(y1, state.ext_config(full, ROW)[:, y1, :])
                w.Evolve()
                tr = scan_rows(w, y1, remove, ref_valid)      # sign of the removal applied; the injection's -1 here
                over.append({y2: -v for y2, v in tr.items()})
        for y2 in range(y1 + 1, rows):
            open_ = ref_valid[:, None] & is_pair[:, y2, :]
            psi = psi_orig[y2]
            if np.any(psi[open_] == 0):
                raise RuntimeError("MeasureSingletPairCorrelation: psi_original = 0 for sampled configuration.")
            safe = np.where(open_, psi, 1.0)
            val = 0.5 * np.conj((over[0][y2] - over[1][y2]) / safe) * tgt_sign[:, y2, :]
            out[:, pos:pos + cols - 1] = np.where(open_, val, 0.0)
            pos += cols - 1
    assert pos == len(mapping)
    return out


# ---- the Hubbard model (square_hubbard_model.h; states 0 = up-down, 1 = up, 2 = down, 3 = empty, :18-23) ----
HUBBARD_NF = (0, 1, 1, 0)                      # fermion parity of each state
_HUB_UP, _HUB_DN = (1, 1, 0, 0), (1, 0, 1, 0)  # HubbardConfig2SpinCounts, square_hubbard_u1u1_updater.h:30-40
_HUB_STATE = {(1, 1): 0, (1, 0): 1, (0, 1): 2, (0, 0): 3}


def hubbard_sector_table():
    """The sector table of pepsgpu_sweep_slice_sector for MCUpdateSquareNNHubbardU1U1OBC, [16][2 + 2 * 4] over physical states: row
    a * 4 + b = (m, init, four slots (a', b')), the pairs with the (N_up, N_down) of (a, b) in the order of
    EnumerateHubbardTwoSiteConfigsWithU1U1 (square_hubbard_u1u1_updater.h:57-72: a' in the outer loop, b' in the inner one), unused
    slots (-1, -1); m is 4, 2 or 1."""
    tab = -np.ones((16, 10), dtype=np.int32)
    for a in range(4):
        for b in range(4):
            nu, nd = _HUB_UP[a] + _HUB_UP[b], _HUB_DN[a] + _HUB_DN[b]
            sector = [(c1, c2) for c1 in range(4) for c2 in range(4)
                      if _HUB_UP[c1] + _HUB_UP[c2] == nu and _HUB_DN[c1] + _HUB_DN[c2] == nd]
            row = tab[a * 4 + b]
            row[0], row[1] = len(sector), sector.index((a, b))
            row[2:2 + 2 * len(sector)] = np.array(sector).ravel()
    return tab


def hubbard_hop_table():
    """The hops of a nearest-neighbour bond of the Hubbard model in the states (a, b), a on the earlier site of the pass's mode order
    (left / upper): (table [16][2][2], signs [16][2]).  Slot 0: the up electron hopped across the bond, slot 1: the down electron; at
    most one hop per spin, (-1, -1) and sign 0 where there is none.  The bond energy is -t sum_k signs[k] conj(psi'_k / psi) with
    s_up = (-1)^(n_down of site 1), s_down = (-1)^(n_up of site 2): the occupation of the one mode the hop passes in the order
    (site 1 up, site 1 down, site 2 up, site 2 down); this is every branch of square_hubbard_model.h:200-262.  The table is the
    hop_table of pepsgpu_nn_hop_slice_fermion."""
    tab = -np.ones((16, 2, 2), dtype=np.int32)
    sign = np.zeros((16, 2), dtype=np.int64)
    for a in range(4):
        for b in range(4):
            ua, da, ub, db = _HUB_UP[a], _HUB_DN[a], _HUB_UP[b], _HUB_DN[b]
            if ua != ub:
                tab[a * 4 + b, 0] = (_HUB_STATE[(ub, da)], _HUB_STATE[(ua, db)])
                sign[a * 4 + b, 0] = 1 - 2 * da
            if da != db:
                tab[a * 4 + b, 1] = (_HUB_STATE[(ua, db)], _HUB_STATE[(ub, da)])
                sign[a * 4 + b, 1] = 1 - 2 * ub
    return tab, sign


def hubbard_observables(ctx, state, configs, t, U, mu=0.0, hop="slice", punch_holes=False):
    """Registry of SquareNNModelMeasurementSolver<SquareHubbardModel>::EvaluateObservables (square_hubbard_model.h:127-171) for a batch
    of configurations, driven from Python: energy [n, 1], charge, spin_z, double_occupancy [n, rows * cols], bond_energy_h / _v.
    Also returns psi_list [rows + cols][n].  The bond energy is EvaluateBondEnergy (:190-262) by the rule of hubbard_hop_table, the
    onsite energy U (#doublons) - mu (#electrons) (:101-117).
    hop = "slice": one pepsgpu_nn_hop_slice_fermion per row / column (punch_holes: the row slices store their holes in HBM);
    "calls": Trace + ReplaceNNSiteTrace per bond."""
    from .capi import LEFT, DOWN, RIGHT, UP, HORIZONTAL, VERTICAL
    if hop not in ("slice", "calls"):
        raise ValueError("hubbard_observables: hop must be 'slice' or 'calls'")
    if tuple(int(x) % 2 for x in state.nf) != HUBBARD_NF:
        raise ValueError("hubbard_observables: the state's parities must be HUBBARD_NF")
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    if rows < 2 or cols < 2:
        raise ValueError("hubbard_observables: the lattice needs at least 2 rows and 2 columns")
    dt = np.complex128 if state.is_complex else np.float64
    table, sign = hubbard_hop_table()
    nf = np.asarray(HUBBARD_NF)
    out = {"h": np.zeros((n, rows, cols - 1), dt), "v": np.zeros((n, rows - 1, cols), dt)}
    psis = []
    for orient, order, approach, step, lo, hi, key in ((HORIZONTAL, ROW, UP, DOWN, LEFT, RIGHT, "h"), (VERTICAL, COL, LEFT, RIGHT, UP, DOWN, "v")):
        S, N = (rows, cols) if orient == HORIZONTAL else (cols, rows)
        ctx.set_configs(state.ext_config(cfg, order))
        ctx.generate_bmps_approach(approach)
        for s in range(S):
            if hop == "slice":
                psi, pr = ctx.nn_hop_slice_fermion(orient, s, nf, table, punch_holes=punch_holes and orient == HORIZONTAL)
            else:
                psi, _, pr = _pair_slice_by_calls(ctx, state, cfg, orient, order, lo, hi, s, table)
            if np.any(psi == 0):
                raise RuntimeError("Wavefunction amplitude is near zero, causing division by zero.")
            psis.append(psi[:, 0])
            for j in range(N - 1):
                (r1, c1), (r2, c2) = ((s, j), (s, j + 1)) if orient == HORIZONTAL else ((j, s), (j + 1, s))
                sg = sign[cfg[:, r1, c1] * 4 + cfg[:, r2, c2]]                  # [n][2]
                out[key][:, r1, c1] = -t * np.sum(sg * np.conj(pr[:, j, :] / psi[:, j, None]), axis=1)
            if s + 1 < S:
                ctx.shift_bmps_window(step)
    doublon = (cfg == 0).astype(np.float64)
    charge = np.asarray(_HUB_UP)[cfg] + np.asarray(_HUB_DN)[cfg]
    energy = out["h"].sum(axis=(1, 2)) + out["v"].sum(axis=(1, 2)) + U * doublon.sum(axis=(1, 2)) - mu * charge.sum(axis=(1, 2))
    return {"energy": energy[:, None], "spin_z": (0.5 * (np.asarray(_HUB_UP)[cfg] - np.asarray(_HUB_DN)[cfg])).reshape(n, -1),
            "charge": charge.astype(np.float64).reshape(n, -1), "double_occupancy": doublon.reshape(n, -1),
            "bond_energy_h": out["h"].reshape(n, -1), "bond_energy_v": out["v"].reshape(n, -1)}, np.array(psis)


def hubbard_energy(ctx, state, configs, t, U, mu=0.0, bonds=None, hop="slice", punch_holes=False):
    """E_loc(S) of H = -t sum_<ij>,s (c+_is c_js + h.c.) + U sum n_up n_down - mu N (square_hubbard_model.h:50-52).  Returns
    (energy [n], psi_list [rows + cols][n]); `bonds` (a dict) receives the per-bond energies "h" and "v"; hop as in
    hubbard_observables."""
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    obs, psis = hubbard_observables(ctx, state, cfg, t, U, mu, hop, punch_holes)
    if bonds is not None:
        bonds.update(h=obs["bond_energy_h"].reshape(n, rows, cols - 1), v=obs["bond_energy_v"].reshape(n, rows - 1, cols))
    return obs["energy"][:, 0], psis


def exact_sum_measure(ctx, state, all_configs, t, V=0.0, rank=0, size=1, batch=None, t2=0.0, tj=None):
    """ExactSumMeasurerMPI (exact_summation_measurer.h:103-257) on the device: configurations rank, rank + size, ... in
    batches of walkers; returns (weighted sums by key, weight sum) -- sum both over ranks (all-reduce) and divide.
    tj = (J, mu): the t-J model's registry (tj_observables with t, V and t2 as given) instead of the spinless one."""
    cfgs = np.asarray(all_configs)[rank::size]
    if len(np.asarray(all_configs)) == 0:
        raise ValueError("ExactSumMeasurerMPI: all_configs must not be empty")
    batch = batch or max(len(cfgs), 1)
    wsum, acc = 0.0, {}
    for b0 in range(0, len(cfgs), batch):
        part = cfgs[b0:b0 + batch]
        if tj is None:
            obs, psis = spinless_fermion_observables(ctx, state, part, t, V, t2)
        else:
            obs, psis = tj_observables(ctx, state, part, t, tj[0], V, tj[1], t2)
        w = np.abs(psis[0]) ** 2                           # |psi(S)|^2: the sign decoration drops out
        wsum += float(w.sum())
        for key, vals in obs.items():
            acc[key] = acc.get(key, 0.0) + w @ vals
    return acc, wsum


def nn_energy(ctx, state, configs, bond_fn, bonds=None):
    """Nearest-neighbour local energy of a fermionic model for every configuration of the batch: the traversal of
    square_nnn_energy_solver.h:116-201 / bond_traversal_mixin.h:113-144 with the fermion interface (psi recomputed
    next to psi').  bond_fn(c1, c2) -> (diagonal energy, coefficient of psi(S with the two states exchanged)/psi(S)),
    arrays over the batch.  Returns (energy [n], psi_list [rows + cols][n]); `bonds` (a dict) receives the per-bond
    energies "h" [n, rows, cols-1] and "v" [n, rows-1, cols] that the measurement registry reports."""
    from .capi import LEFT, DOWN, RIGHT, UP, HORIZONTAL, VERTICAL
    cfg = np.asarray(configs)
    n, rows, cols = cfg.shape
    dt = np.complex128 if state.is_complex else np.float64       # QLTEN_Complex: E_loc = sum H conj(psi' / psi) (the reference's ComplexConjugate)
    e = np.zeros(n, dt)
    psis = []
    if bonds is not None:
        bonds.update(h=np.zeros((n, rows, cols - 1), dt), v=np.zeros((n, rows - 1, cols), dt))

    def bond(s1, s2, orient, order, ext):
        (r1, c1), (r2, c2) = s1, s2
        e_int, off = bond_fn(cfg[:, r1, c1], cfg[:, r2, c2])
        e_int = np.broadcast_to(np.asarray(e_int, dtype=np.float64), (n,))
        off = np.broadcast_to(np.asarray(off, dtype=np.float64), (n,))
        differ = off != 0.0
        if not differ.any():
            return e_int
        psi = ctx.trace(r1, c1, orient)                       # psi along the same path as psi' (sign consistency)
        new = cfg.copy()
        new[:, r1, c1], new[:, r2, c2] = cfg[:, r2, c2], cfg[:, r1, c1]
        ne = state.ext_config(new, order)
        cand = np.stack([ne[:, r1, c1], ne[:, r2, c2]], axis=-1)[:, None, :]
        psi_ex = ctx.replace_nn_trace(r1, c1, orient, cand)[:, 0]
        return e_int + np.where(differ, off * np.conj(psi_ex / np.where(psi == 0, 1.0, psi)), 0.0)

    ext = state.ext_config(cfg, ROW)
    ctx.set_configs(ext)
    ctx.generate_bmps_approach(UP)
    for row in range(rows):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        psis.append(ctx.trace(row, 0, HORIZONTAL))
        for col in range(cols - 1):
            eb = bond((row, col), (row, col + 1), HORIZONTAL, ROW, ext)
            e += eb
            if bonds is not None:
                bonds["h"][:, row, col] = eb
            ctx.shift_bten_window(RIGHT)
        if row < rows - 1:
            ctx.shift_bmps_window(DOWN)
    ext = state.ext_config(cfg, COL)
    ctx.set_configs(ext)
    ctx.generate_bmps_approach(LEFT)
    for col in range(cols):
        ctx.init_bten(UP, col)
        ctx.grow_full_bten(DOWN, col, 2, True)
        psis.append(ctx.trace(0, col, VERTICAL))
        for row in range(rows - 1):
            eb = bond((row, col), (row + 1, col), VERTICAL, COL, ext)
            e += eb
            if bonds is not None:
                bonds["v"][:, row, col] = eb
            if row < rows - 2:
                ctx.shift_bten_window(DOWN)
        if col < cols - 1:
            ctx.shift_bmps_window(RIGHT)
    return e, np.array(psis)


def random_even_state(rows, cols, D, seed, n_odd=None, background=1.0, noise=0.1):
    """synthetic fermionic state for throughput / parity runs (the reference ships no fermionic state larger
    than 2x2): bond space = D states of which n_odd (default D // 2) are odd, site tensors N(0,1) on the
    parity-even entries plus a positive background on the all-even entry; state 0 occupied, 1 empty."""
    rng = np.random.default_rng(seed)
    n_odd = D // 2 if n_odd is None else n_odd
    bond = np.r_[np.zeros(D - n_odd, dtype=np.int64), np.ones(n_odd, dtype=np.int64)]
    one = np.zeros(1, dtype=np.int64)
    tensors, par = [[None] * cols for _ in range(rows)], [[None] * cols for _ in range(rows)]
    for r in range(rows):
        for c in range(cols):
            p = (one if c == 0 else bond, one if r == rows - 1 else bond, one if c == cols - 1 else bond, one if r == 0 else bond)
            par[r][c] = p
            tot = p[0][:, None, None, None] + p[1][None, :, None, None] + p[2][None, None, :, None] + p[3][None, None, None, :]
            comp = []
            for s, n in enumerate((1, 0)):
                # smooth positive background on the parity-allowed entries + noise (as the bosonic generator of
                # SURVEY 8d): keeps the network well conditioned so that chi-truncation is meaningful
                vec = [rng.uniform(0.5, 1.5, size=k) for k in tot.shape]
                bg = vec[0][:, None, None, None] * vec[1][None, :, None, None] * vec[2][None, None, :, None] * vec[3][None, None, None, :]
                a = (background * bg + noise * rng.standard_normal(tot.shape)) * ((tot + n) % 2 == 0)
                comp.append(a / np.sqrt(max(1.0, np.sum(a * a))) * 2.0)
            tensors[r][c] = comp
    return FermionState(tensors, par, [1, 0])
