"""What a tensor-GEMM descriptor means (peps_amd/csrc/tgemm.h TGemmDesc), restated in float64 / complex128 NumPy.

The descriptor is the dict peps_amd.capi.tgemm_desc_arrays takes (keys as the TGemmDesc fields, per-batch arrays as integer
sequences, a TgDyn as desc["dI1"] = dict(p=..., mul=, mask=, div=)).  Every rule below cites the tgemm.h line it restates.
The reference runs over one batch entry at a time; the shapes of the kernel tests are small.
"""
import numpy as np


def _dyn(desc, key):
    t = desc.get(key) or {}
    return t.get("p"), int(t.get("mul", 1)), int(t.get("mask", 0)), int(t.get("div", 1))


def live_extents(desc, b):
    """(I, J, K, Imask, Jmask, Itot, Ktot) of batch entry b after its per-walker extents are applied."""
    I, J, K = list(desc.get("I", (1, 1, 1))), list(desc.get("J", (1, 1, 1))), list(desc.get("K", (1, 1, 1)))
    big = 0x7FFFFFFF
    Imask, Jmask = [big] * 3, [big] * 3
    for s in range(3):
        # extent of sub-index s = max(0, min(static, p[b / div] * mul)); mask = 1 keeps the static tiling and masks the
        # index instead of compacting it (tgemm.h:22-31, applied at :471-473 / :502-504 / :542-544)
        for dims, mask, key in ((I, Imask, "dI%d" % s), (J, Jmask, "dJ%d" % s), (K, None, "dK%d" % s)):
            p, mul, msk, div = _dyn(desc, key)
            if p is None:
                continue
            e = max(0, min(dims[s], int(p[b // div]) * mul))
            if msk and mask is not None:
                mask[s] = e
            else:
                dims[s] = e       # (dK has no mask: tgemm.h:473 / :504 / :544)
    Itot = I[0] * I[1] * I[2]
    Ktot = K[0] * K[1] * K[2]
    # dynI / dynK: only the first dyn[b] * mul values of the flattened index exist (tgemm.h:44-47, :477-478 / :508-509 / :892)
    if desc.get("dynI") is not None:
        Itot = max(0, min(Itot, int(desc["dynI"][b]) * int(desc.get("dynI_mul", 1))))
    if desc.get("dynK") is not None:
        Ktot = max(0, min(Ktot, int(desc["dynK"][b]) * int(desc.get("dynK_mul", 1))))
    return I, J, K, Imask, Jmask, Itot, Ktot


def _split(idx, dims):
    """flattened index -> sub-indices, innermost last (tgemm.h:90-105 tg_off3 / tg_off3m)."""
    i2 = idx % dims[2]
    r = idx // dims[2]
    return r // dims[1], r % dims[1], i2


def _offsets(n, dims, strides, lim=None):
    idx = np.arange(n, dtype=np.int64)
    i0, i1, i2 = _split(idx, dims)
    off = i0 * strides[0] + i1 * strides[1] + i2 * strides[2]
    if lim is None:
        return off, np.ones(n, dtype=bool)
    # a sub-index at or beyond its mask limit: the operand reads as zero there (tgemm.h:95, :616-617)
    return off, (i0 < lim[0]) & (i1 < lim[1]) & (i2 < lim[2])


def operand_bases(desc, b):
    """(base of A, base of B, base of C) of entry b: (b / bdiv) * w + sel[(b / seldiv) * inc] * mul
    (tgemm.h:39-43, :124-129 / :347-352 / :902-904)."""
    g = desc.get
    bA = (b // int(g("bdivA", 1))) * int(g("wA", 0))
    bB = (b // int(g("bdivB", 1))) * int(g("wB", 0))
    bC = (b // int(g("bdivC", 1))) * int(g("wC", 0))
    if g("selA") is not None:
        bA += int(g("selA")[(b // int(g("seldivA", 1))) * int(g("selA_inc", 0))]) * int(g("selA_mul", 0))
    if g("selB") is not None:
        bB += int(g("selB")[(b // int(g("seldivB", 1))) * int(g("selB_inc", 0))]) * int(g("selB_mul", 0))
    return bA, bB, bC


def entry_index_sets(desc, b):
    """The element offsets entry b reads: (A offsets [Itot, Ktot] of the rows that exist, B offsets [Ktot, Jtot] of the columns
    that exist), relative to the start of the buffers (before the caller's pointer offsets)."""
    I, J, K, Imask, Jmask, Itot, Ktot = live_extents(desc, b)
    Jtot = J[0] * J[1] * J[2]
    bA, bB, _ = operand_bases(desc, b)
    g = desc.get
    oAi, liveI = _offsets(Itot, I, g("sAi"), Imask)
    oAk, _ = _offsets(Ktot, K, g("sAk"))
    oBk, _ = _offsets(Ktot, K, g("sBk"))
    oBj, liveJ = _offsets(Jtot, J, g("sBj"), Jmask)
    a = bA + oAi[liveI][:, None] + oAk[None, :]
    bo = bB + oBk[:, None] + oBj[liveJ][None, :]
    return a, bo


def tgemm_ref(desc, A, B, C0, a_offset=0, b_offset=0, scale_in=None):
    """Reference of one tgemm_launch.  A, B, C0 are the flat buffers the diagnostic uploads (A is read from A[a_offset:]).

    Returns dict(C=expected C (float64 / complex128), written=bool mask of the elements the launch must store,
    lower=bool mask of the elements strictly below the diagonal of an upper_only launch (stored or left as they were),
    absprod=alpha-scaled (|op(A)| |op(B)|)_ij + |C0| where written (the scale of the rounding error), K=live K per element,
    flops=the launch's flop count, norm=per-entry 2-norm of what is stored (fused normalisation)).
    """
    g = desc.get
    cplx = np.iscomplexobj(A) or np.iscomplexobj(B)
    ft = np.complex128 if cplx else np.float64
    Aw = np.asarray(A, dtype=ft)[a_offset:]
    Bw = np.asarray(B, dtype=ft)[b_offset:]
    C = np.array(C0, dtype=ft, copy=True)
    written = np.zeros(C.shape, dtype=bool)
    lower = np.zeros(C.shape, dtype=bool)
    absprod = np.zeros(C.shape, dtype=np.float64)
    kl = np.zeros(C.shape, dtype=np.int64)
    nb = int(g("nbatch", 1))
    flops = 0
    norms = np.zeros(nb)
    alpha = float(g("alpha", 1.0))
    for b in range(nb):
        # batch_flag[b] >= 0: the entry is skipped, C[b] untouched (tgemm.h:55, :468 / :499 / :887)
        if g("batch_flag") is not None and int(g("batch_flag")[b]) >= 0:
            continue
        I, J, K, Imask, Jmask, Itot, Ktot = live_extents(desc, b)
        Jtot = J[0] * J[1] * J[2]
        if Itot <= 0 or Jtot <= 0:
            continue
        flops += (1 if g("upper_only") else 2) * Itot * Jtot * Ktot       # (tgemm.h:480 / :512 / :899: the tiled extents)
        bA, bB, bC = operand_bases(desc, b)
        oAi, liveI = _offsets(Itot, I, g("sAi"), Imask)
        oAk, _ = _offsets(Ktot, K, g("sAk"))
        oBk, _ = _offsets(Ktot, K, g("sBk"))
        oBj, liveJ = _offsets(Jtot, J, g("sBj"), Jmask)
        oCi, _ = _offsets(Itot, I, g("sCi"))
        oCj, _ = _offsets(Jtot, J, g("sCj"))
        Am = np.zeros((Itot, Ktot), dtype=ft)
        Bm = np.zeros((Ktot, Jtot), dtype=ft)
        Am[liveI] = Aw[bA + oAi[liveI][:, None] + oAk[None, :]]
        Bm[:, liveJ] = Bw[bB + oBk[:, None] + oBj[liveJ][None, :]]
        # conjA / conjB: the complex operand enters conjugated (tgemm.h:54, :211-214)
        if g("conjA"):
            Am = np.conj(Am)
        if g("conjB"):
            Bm = np.conj(Bm)
        # C = alpha * op(A) op(B) (+ C) (tgemm.h:288-297 / :446-461); scale_in[b] multiplies alpha (tgemm.h:592, :908-911)
        a_eff = alpha * (float(scale_in[b]) if (g("scale_in") and scale_in is not None) else 1.0)
        with np.errstate(invalid="ignore"):       # (an entry holding an infinity: its products are inf or NaN)
            P = a_eff * (Am @ Bm)
            absP = abs(a_eff) * (np.abs(Am) @ np.abs(Bm))
        cidx = bC + oCi[:, None] + oCj[None, :]
        old = C[cidx]
        new = P + old if g("accumulate") else P
        C[cidx] = new
        written[cidx] = True
        absprod[cidx] = absP + (np.abs(old) if g("accumulate") else 0.0)
        kl[cidx] = Ktot
        norms[b] = np.sqrt(np.sum(np.abs(new) ** 2))
        if g("upper_only"):
            # tiles of 64 x 64 strictly below the diagonal are not computed (tgemm.h:53, :519): what lies below the diagonal
            # is either untouched or correct
            ii = np.arange(Itot)[:, None]
            jj = np.arange(Jtot)[None, :]
            lower[cidx] = ii > jj
    return dict(C=C, written=written, lower=lower, absprod=absprod, K=kl, flops=flops, norm=norms)


def fused_norm_ref(norm, norm_log0):
    """scale_out = float32(1 / |C_b|), norm_log -= log(scale_out as stored); a zero or non-finite norm: scale 1 and flag 1,
    norm_log unchanged (tgemm.h:60-68, :894, :919-931)."""
    norm = np.asarray(norm, dtype=np.float64)
    ok = (norm > 0) & np.isfinite(norm)
    so = np.where(ok, (1.0 / np.where(ok, norm, 1.0)).astype(np.float32), np.float32(1.0)).astype(np.float32)
    nl = np.asarray(norm_log0, dtype=np.float64) - np.where(ok, np.log(so.astype(np.float64)), 0.0)
    nf = np.where(ok, 0, 1).astype(np.int32)
    return so, nl, nf
