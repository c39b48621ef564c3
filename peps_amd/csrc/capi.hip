// extern "C" boundary of libpepsgpu.so (declared in include/pepsgpu.h).
#include <cstring>
#include "../../include/pepsgpu.h"
#include "engine_impl.h"
#include "engine_nnn.h"
#include "engine_sr.h"
#include "engine_opt.h"
#include "engine_lbfgs.h"
#include "engine_guard.h"
#include "engine_var.h"
#include "engine_cplx.h"
#include "engine_walker.h"
#include "engine_sweep.h"
#include "comm.h"

using namespace pepsgpu;

namespace pepsgpu {
bool tgemm_use_mfma() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("PEPSGPU_NO_MFMA");
    v = (e && e[0] == '1') ? 0 : 1;
  }
  return v == 1;
}
}  // namespace pepsgpu

struct pepsgpu_ctx {
  EngineBase *eng = nullptr;
  Comm comm;
  std::string err;
};

static thread_local std::string g_err;

template <typename F>
static int guarded(pepsgpu_ctx *ctx, F &&f) {
  try {
    f();
    return PEPSGPU_OK;
  } catch (const Error &e) {
    if (ctx) ctx->err = e.what(); else g_err = e.what();
    return e.code;
  } catch (const std::exception &e) {
    if (ctx) ctx->err = e.what(); else g_err = e.what();
    return PEPSGPU_EHIP;
  }
}

// every entry makes the context's GPU the calling thread's current device first: a context is bound to one device, the
// caller (another context, torch, another thread) may have changed the thread's device since the last call
#define CTX_CALL(body)                                     \
  if (!ctx || !ctx->eng) return PEPSGPU_EINVAL;            \
  return guarded(ctx, [&]() { PG_CHECK_HIP(hipSetDevice(ctx->eng->device_id)); body; })

struct DevBufs {     // device allocations of one diagnostic call, freed on every exit
  std::vector<void *> p;
  template <typename T> T *alloc(size_t n, const void *init = nullptr) {
    void *q = nullptr;
    PG_CHECK_HIP(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    p.push_back(q);
    if (init && n) PG_CHECK_HIP(hipMemcpy(q, init, n * sizeof(T), hipMemcpyHostToDevice));
    return (T *)q;
  }
  ~DevBufs() { for (void *q : p) (void)hipFree(q); }
};

static void diag_eigh_impl(hipStream_t s, int n, int is_complex, const double *a, double *w_out, double *z_out, int *sweeps_out) {
  PG_REQUIRE(n >= 1 && a && w_out && z_out, 1, "diag_eigh: n < 1 or a null buffer");
  const int Z = is_complex ? 2 : 1;
  const size_t nn = (size_t)n * n * Z;
  for (size_t e = 0; e < nn; ++e) PG_REQUIRE(std::isfinite(a[e]), 1, "diag_eigh: non-finite input");
  DevBufs bufs;
  double *da = bufs.alloc<double>(nn, a), *dv = bufs.alloc<double>(nn), *dw = bufs.alloc<double>(n);
  double *work = bufs.alloc<double>(eigh_work_doubles(n));
  int sweeps = 0;
  const bool converged = eigh_jacobi(s, n, is_complex != 0, da, dv, dw, work, &sweeps);
  PG_CHECK_HIP(hipStreamSynchronize(s));
  if (sweeps_out) *sweeps_out = sweeps;
  std::vector<double> zt(nn);
  PG_CHECK_HIP(hipMemcpy(zt.data(), da, nn * sizeof(double), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(w_out, dw, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  for (int r = 0; r < n; ++r)          // the device keeps Z^T: row k = the eigenvector of w[k]
    for (int k = 0; k < n; ++k)
      for (int z = 0; z < Z; ++z) z_out[Z * ((size_t)r * n + k) + z] = zt[Z * ((size_t)k * n + r) + z];
  if (!converged) throw Error(PEPSGPU_ENOCONV, "diag_eigh: the Jacobi eigensolver reached its sweep cap");
}

extern "C" {

const char *pepsgpu_version(void) { return "pepsgpu 0.1 (gfx950)"; }

int pepsgpu_ctx_create(pepsgpu_ctx **out, int device, int dtype, int rows, int cols, int D, int phys_dim,
                       int chi_min, int chi_max, double trunc_err, int scheme, int max_walkers) {
  if (!out) return PEPSGPU_EINVAL;
  *out = nullptr;
  pepsgpu_ctx *ctx = new pepsgpu_ctx;
  int rc = guarded(nullptr, [&]() {
    PG_REQUIRE(scheme >= PEPSGPU_SVD_COMPRESS && scheme <= PEPSGPU_VARIATION1SITE, 1, "unknown CompressMPSScheme");
    PG_REQUIRE(chi_min <= chi_max, 1, "D_min > D_max");
    int ndev = 0;
    PG_CHECK_HIP(hipGetDeviceCount(&ndev));
    PG_REQUIRE(ndev > 0 && device >= 0 && device < ndev, 2, "no such HIP device");
    // walkers x candidates is the z extent of the contraction grids (65535); refuse here, not at the first launch
    PG_REQUIRE(max_walkers >= 1 && max_walkers <= 65535, 1, "max_walkers must be in [1, 65535] (grid z limit)");
    if (dtype == PEPSGPU_F32)
      ctx->eng = new Engine<float>(device, rows, cols, D, phys_dim, chi_min, chi_max, trunc_err, max_walkers);
    else if (dtype == PEPSGPU_F64)
      ctx->eng = new Engine<double>(device, rows, cols, D, phys_dim, chi_min, chi_max, trunc_err, max_walkers);
    else if (dtype == PEPSGPU_C128)
      ctx->eng = new Engine<c128>(device, rows, cols, D, phys_dim, chi_min, chi_max, trunc_err, max_walkers);
    else
      throw Error(1, "unknown dtype");
    // variational schemes: convergence_tol / iter_max default to 1e-10 / 10 until pepsgpu_set_truncate_params sets them
    if (scheme != PEPSGPU_SVD_COMPRESS) ctx->eng->set_truncate_params(chi_min, chi_max, trunc_err, scheme, 1e-10, 10);
  });
  if (rc != PEPSGPU_OK) {
    delete ctx;
    return rc;
  }
  *out = ctx;
  return PEPSGPU_OK;
}

int pepsgpu_set_truncate_params(pepsgpu_ctx *ctx, int chi_min, int chi_max, double trunc_err, int scheme,
                                double convergence_tol, int iter_max) {
  CTX_CALL(ctx->eng->set_truncate_params(chi_min, chi_max, trunc_err, scheme, convergence_tol, iter_max));
}

void pepsgpu_ctx_destroy(pepsgpu_ctx *ctx) {
  if (!ctx) return;
  if (ctx->eng) (void)hipSetDevice(ctx->eng->device_id);
  ctx->comm.destroy();
  delete ctx->eng;
  delete ctx;
}

const char *pepsgpu_last_error(pepsgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int pepsgpu_state_upload(pepsgpu_ctx *ctx, const void *p, int host_dtype) {
  CTX_CALL(PG_REQUIRE(p != nullptr, 1, "null state buffer"); ctx->eng->state_upload(p, host_dtype));
}
int pepsgpu_walkers_set_configs(pepsgpu_ctx *ctx, int n, const int32_t *cfg) {
  CTX_CALL(PG_REQUIRE(cfg != nullptr, 1, "null configuration buffer"); ctx->eng->set_configs(n, cfg));
}
int pepsgpu_walkers_get_configs(pepsgpu_ctx *ctx, int32_t *out) { CTX_CALL(ctx->eng->get_configs(out)); }
int pepsgpu_n_walkers(pepsgpu_ctx *ctx) { return (ctx && ctx->eng) ? ctx->eng->n_walkers() : -1; }

static void check_pos(int pos) { PG_REQUIRE(pos >= 0 && pos < 4, 1, "bad BMPSPOSITION"); }

int pepsgpu_grow_bmps_step(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->grow_bmps_step(pos)); }
int pepsgpu_grow_full_bmps(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->grow_full_bmps(pos)); }
int pepsgpu_grow_bmps_for_row(pepsgpu_ctx *ctx, int row) { CTX_CALL(ctx->eng->grow_bmps_for_row(row)); }
int pepsgpu_grow_bmps_for_col(pepsgpu_ctx *ctx, int col) { CTX_CALL(ctx->eng->grow_bmps_for_col(col)); }
int pepsgpu_shift_bmps_window(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->shift_bmps_window(pos)); }
int pepsgpu_delete_inner_bmps(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->delete_inner_bmps(pos)); }
int pepsgpu_sweep_slice_exchange(pepsgpu_ctx *ctx, int orientation, int slice, int n_uniform, const double *uniforms,
                                 double *amplitude_inout, int32_t *consumed_out, int32_t *accepted_out, int32_t *slice_states_out) {
  CTX_CALL(PG_REQUIRE(uniforms && amplitude_inout && consumed_out && accepted_out, 1, "null buffer");
           ctx->eng->sweep_slice_exchange(orientation, slice, n_uniform, uniforms, nullptr, amplitude_inout, consumed_out, accepted_out,
                                          slice_states_out));
}
int pepsgpu_sweep_slice_exchange_tab(pepsgpu_ctx *ctx, int orientation, int slice, int n_uniform, const double *uniforms,
                                     const int32_t *pair_table, double *amplitude_inout, int32_t *consumed_out, int32_t *accepted_out,
                                     int32_t *slice_states_out) {
  CTX_CALL(PG_REQUIRE(uniforms && amplitude_inout && consumed_out && accepted_out, 1, "null buffer");
           ctx->eng->sweep_slice_exchange(orientation, slice, n_uniform, uniforms, pair_table, amplitude_inout, consumed_out, accepted_out,
                                          slice_states_out));
}
int pepsgpu_sweep_slice_fullspace(pepsgpu_ctx *ctx, int orientation, int slice, int phys_dim, const uint32_t *engine_words,
                                  double *amplitude_inout, int32_t *accepted_out, int32_t *slice_states_out) {
  CTX_CALL(PG_REQUIRE(engine_words && amplitude_inout && accepted_out, 1, "null buffer");
           ctx->eng->sweep_slice_fullspace(orientation, slice, phys_dim, engine_words, amplitude_inout, accepted_out, slice_states_out));
}
// the bosonic triple table pepsgpu_sweep_slice_tnn3 builds for a NULL table (host only, no context)
int pepsgpu_diag_tnn3_table(int phys_dim, int32_t *out) {
  if (phys_dim < 1 || phys_dim > 64 || !out) return PEPSGPU_EINVAL;
  const std::vector<int32_t> tab = pepsgpu::tnn3_boson_table(phys_dim);
  std::copy(tab.begin(), tab.end(), out);
  return 0;
}
// square_3site_updater.h:36-56 / :61-81 (one slice of MCUpdateSquareTNN3SiteUpdateBase::operator()) + :109-158 per triple
int pepsgpu_sweep_slice_tnn3(pepsgpu_ctx *ctx, int orientation, int slice, const int32_t *triple_table, int n_words,
                             const uint32_t *engine_words, double *amplitude_out, int32_t *consumed_out, int32_t *accepted_out,
                             int32_t *slice_states_out) {
  CTX_CALL(PG_REQUIRE(engine_words && amplitude_out && consumed_out && accepted_out, 1, "null buffer");
           ctx->eng->sweep_slice_tnn3(orientation, slice, triple_table, n_words, engine_words, amplitude_out, consumed_out,
                                      accepted_out, slice_states_out));
}
int pepsgpu_nn_exchange_slice(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, double *psi_out, double *psi_exchanged_out) {
  CTX_CALL(PG_REQUIRE(psi_out && psi_exchanged_out, 1, "null buffer");
           ctx->eng->nn_exchange_slice(orientation, slice, punch_holes, psi_out, psi_exchanged_out));
}
int pepsgpu_nn_exchange_slice_tab(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, const int32_t *pair_table,
                                  int psi_per_bond, double *psi_out, double *psi_exchanged_out) {
  CTX_CALL(PG_REQUIRE(psi_out && psi_exchanged_out, 1, "null buffer");
           ctx->eng->energy_slice_impl(0, orientation, slice, punch_holes, pair_table, 1, psi_per_bond, psi_out, psi_exchanged_out));
}
int pepsgpu_onsite_slice(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, int n_cand, const int32_t *site_table,
                         double *psi_out, double *psi_cand_out) {
  CTX_CALL(PG_REQUIRE(site_table && psi_out && psi_cand_out, 1, "null buffer"); PG_REQUIRE(n_cand >= 1, 1, "n_cand < 1");
           ctx->eng->energy_slice_impl(1, orientation, slice, punch_holes, site_table, n_cand, 0, psi_out, psi_cand_out));
}
// square_nnn_energy_solver.h:203-265: the diagonal bonds of one row pair
int pepsgpu_nnn_exchange_slice(pepsgpu_ctx *ctx, int row1, int diag_mask, double *val_out) {
  CTX_CALL(PG_REQUIRE(val_out, 1, "null buffer"); ctx->eng->nnn_exchange_slice(row1, diag_mask, val_out));
}
long pepsgpu_diag_nnn_slice_calls(void) { return pepsgpu::nnn_slice_calls().load(); }
// square_spinless_fermion.h:161-200 / square_tJ_model.h:424-463: the diagonal hops of one row pair of a fermionic state
int pepsgpu_nnn_hop_slice_fermion(pepsgpu_ctx *ctx, int row1, int d, const int32_t *occ, int diag_mask, double *psi_out, double *val_out) {
  CTX_CALL(PG_REQUIRE(occ && psi_out && val_out, 1, "null buffer");
           ctx->eng->nnn_hop_slice_fermion(row1, d, occ, diag_mask, psi_out, val_out));
}
long pepsgpu_diag_nnn_hop_slice_calls(void) { return pepsgpu::nnn_hop_slice_calls().load(); }
// nnn_hop_cand_kernel alone on a caller's extended configurations ext [n][rows][cols] (row-major variants 0 / 1), for the plaquette
// (row1, col1): cand_out [n][2][4], sign_out [n][2], flag_out [n][2], entry 0 LEFTUP_TO_RIGHTDOWN, entry 1 LEFTDOWN_TO_RIGHTUP
int pepsgpu_diag_fermion_hop_cand(int rows, int cols, int d, const int32_t *occ, int n, const int32_t *ext, int row1, int col1,
                                  int32_t *cand_out, int32_t *sign_out, int32_t *flag_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(occ && ext && cand_out && sign_out && flag_out, 1, "null buffer");
    PG_REQUIRE(rows >= 2 && cols >= 2 && n >= 1 && (double)n * rows * cols < 2147483648.0, 1, "bad sizes");
    PG_REQUIRE(row1 >= 0 && row1 + 1 < rows && col1 >= 0 && col1 + 1 < cols, 1, "plaquette outside the lattice");
    const unsigned occ_bits = pepsgpu::hop_occ_bits(d, occ);
    const int sites = rows * cols;
    const size_t ne = (size_t)n * sites;
    for (size_t e = 0; e < ne; ++e) PG_REQUIRE(ext[e] >= 0 && ext[e] < 2 * d, 1, "extended state outside [0, 2 d)");
    DevBufs m;
    const int *dcfg = m.alloc<int>(ne, ext);
    int *dc = m.alloc<int>(12 * (size_t)n), *ds = dc + 8 * (size_t)n, *df = dc + 10 * (size_t)n;
    const int s0 = row1 * cols + col1, s1 = s0 + cols, s2 = s1 + 1, s3 = s0 + 1;
    hipLaunchKernelGGL(nnn_hop_cand_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, 0, dcfg, sites, s0, s1, s2, s3, d, occ_bits,
                       2, (int)LEFTUP_TO_RIGHTDOWN, (int)LEFTDOWN_TO_RIGHTUP, (int *)nullptr, dc, df, ds, 2L, n);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(cand_out, dc, 8 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(sign_out, ds, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(flag_out, df, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  });
}
// square_tJ_model.h:546-603 next to :301-345: psi, the exchanged amplitude and the pair candidates of every bond of one row / column
int pepsgpu_nn_pair_slice_fermion(pepsgpu_ctx *ctx, int orientation, int slice, int d, const int32_t *occ, const int32_t *pair_table,
                                  const int32_t *exchange_table, double *psi_out, double *ex_out, double *pair_out) {
  CTX_CALL(PG_REQUIRE(occ && pair_table && psi_out && pair_out && (!exchange_table || ex_out), 1, "null buffer");
           ctx->eng->nn_pair_slice_fermion(orientation, slice, d, occ, pair_table, exchange_table, psi_out, ex_out, pair_out));
}
long pepsgpu_diag_pair_slice_calls(void) { return pepsgpu::pair_slice_calls().load(); }
// pair_cand_kernel alone on a caller's extended configurations ext [n][rows][cols] for the bond (site1, site2), flat row-major indices
// of the left / upper and the right / lower site: cand_out [n][2][2], sign_out [n][2]
int pepsgpu_diag_pair_cand(int rows, int cols, int d, const int32_t *occ, const int32_t *pair_table, int n, const int32_t *ext,
                           int orientation, int site1, int site2, int32_t *cand_out, int32_t *sign_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(occ && pair_table && ext && cand_out && sign_out, 1, "null buffer");
    PG_REQUIRE(orientation == HORIZONTAL || orientation == VERTICAL, 1, "bad orientation");
    PG_REQUIRE(rows >= 1 && cols >= 1 && n >= 1 && (double)n * rows * cols < 2147483648.0, 1, "bad sizes");
    const bool hor = orientation == HORIZONTAL;
    const int sites = rows * cols;
    PG_REQUIRE(site1 >= 0 && site2 < sites && site2 == site1 + (hor ? 1 : cols) && (!hor || site1 % cols + 1 < cols), 1,
               "the two sites are no bond of this orientation");
    const unsigned occ_bits = pepsgpu::require_pair_tables(d, occ, pair_table);
    const size_t ne = (size_t)n * sites;
    for (size_t e = 0; e < ne; ++e) PG_REQUIRE(ext[e] >= 0 && ext[e] < 4 * d, 1, "extended state outside [0, 4 d)");
    for (int w = 0; w < n; ++w)
      for (int s : {site1, site2})
        PG_REQUIRE((ext[(size_t)w * sites + s] / d >= 2) == !hor, 1, "extended states of the other mode order on the bond");
    DevBufs m;
    const int *dcfg = m.alloc<int>(ne, ext);
    const int *dtab = m.alloc<int>(4 * (size_t)d * d, pair_table);
    int *dc = m.alloc<int>(6 * (size_t)n), *ds = dc + 4 * (size_t)n;
    hipLaunchKernelGGL(pair_cand_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dcfg, sites, site1, site2, d, occ_bits, hor ? 0 : 1, dtab,
                       (const int *)nullptr, 4 * d, dc, (int *)nullptr, ds, n);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(cand_out, dc, 4 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(sign_out, ds, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  });
}
// square_hubbard_model.h:200-262: psi and the two hopped amplitudes of every bond of one row / column, with the holes of the row pass
int pepsgpu_nn_hop_slice_fermion(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, int d, const int32_t *occ,
                                 const int32_t *hop_table, double *psi_out, double *hop_out) {
  CTX_CALL(PG_REQUIRE(occ && hop_table && psi_out && hop_out, 1, "null buffer");
           ctx->eng->nn_hop_slice_fermion(orientation, slice, punch_holes, d, occ, hop_table, psi_out, hop_out));
}
long pepsgpu_diag_hop_slice_calls(void) { return pepsgpu::hop_slice_calls().load(); }
// square_nn_updater.h:41-55 / :62-76 (one slice of MCUpdateSquareNNUpdateBaseOBC::operator()) + square_hubbard_u1u1_updater.h:95-157
// per bond
int pepsgpu_sweep_slice_sector(pepsgpu_ctx *ctx, int orientation, int slice, int d, const int32_t *occ, int max_cand,
                               const int32_t *sector_table, int n_words, const uint32_t *engine_words, double *amplitude_inout,
                               int32_t *consumed_out, int32_t *accepted_out, int32_t *slice_states_out) {
  CTX_CALL(PG_REQUIRE(sector_table && engine_words && amplitude_inout && consumed_out && accepted_out, 1, "null buffer");
           ctx->eng->sweep_slice_sector(orientation, slice, d, occ, max_cand, sector_table, n_words, engine_words, amplitude_inout,
                                        consumed_out, accepted_out, slice_states_out));
}
long pepsgpu_diag_sector_slice_calls(void) { return pepsgpu::sector_slice_calls().load(); }
// sector_cand_kernel alone on a caller's configurations ext [n][rows][cols] for the bond (site1, site2), flat row-major indices of the
// left / upper and the right / lower site: cand_out [n][max_cand][2], meta_out [n][2] = (m, init).  occ NULL: a bosonic table over
// states in [0, d); else extended states in [0, 4 d) of the mode order of `orientation` on the two sites
int pepsgpu_diag_sector_cand(int rows, int cols, int d, const int32_t *occ, int max_cand, const int32_t *sector_table, int n,
                             const int32_t *ext, int orientation, int site1, int site2, int32_t *cand_out, int32_t *meta_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(sector_table && ext && cand_out && meta_out, 1, "null buffer");
    PG_REQUIRE(orientation == HORIZONTAL || orientation == VERTICAL, 1, "bad orientation");
    PG_REQUIRE(rows >= 1 && cols >= 1 && n >= 1 && (double)n * rows * cols < 2147483648.0, 1, "bad sizes");
    const bool hor = orientation == HORIZONTAL;
    const int sites = rows * cols;
    PG_REQUIRE(site1 >= 0 && site2 < sites && site2 == site1 + (hor ? 1 : cols) && (!hor || site1 % cols + 1 < cols), 1,
               "the two sites are no bond of this orientation");
    const unsigned occ_bits = pepsgpu::require_sector_table(d, occ, max_cand, sector_table);
    const int dp = occ ? 4 * d : d;
    const size_t ne = (size_t)n * sites;
    for (size_t e = 0; e < ne; ++e) PG_REQUIRE(ext[e] >= 0 && ext[e] < dp, 1, "state outside the physical dimension");
    if (occ)
      for (int w = 0; w < n; ++w)
        for (int s : {site1, site2})
          PG_REQUIRE((ext[(size_t)w * sites + s] / d >= 2) == !hor, 1, "extended states of the other mode order on the bond");
    PG_REQUIRE((double)n * max_cand < 1073741824.0, 1, "bad sizes");
    DevBufs m;
    const int *dcfg = m.alloc<int>(ne, ext);
    const int *dtab = m.alloc<int>((size_t)d * d * pepsgpu::sector_row_len(max_cand), sector_table);
    int *dc = m.alloc<int>((2 * (size_t)max_cand + 2) * n), *dm = dc + 2 * (size_t)max_cand * n;
    hipLaunchKernelGGL(sector_cand_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dcfg, sites, site1, site2, d, occ_bits,
                       !occ ? 0 : hor ? 1 : 2, dtab, max_cand, dc, dm, n);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(cand_out, dc, 2 * (size_t)max_cand * n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(meta_out, dm, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  });
}
// spin_onehalf_triangle_heisenbergJ1J2_sqrpeps.h:350-398 / :425-442: the links of one row pair / column pair
int pepsgpu_link_exchange_slice(pepsgpu_ctx *ctx, int orient, int slice1, int link_mask, double *val_out) {
  CTX_CALL(PG_REQUIRE(val_out, 1, "null buffer"); ctx->eng->link_exchange_slice(orient, slice1, link_mask, val_out));
}
long pepsgpu_diag_link_slice_calls(void) { return pepsgpu::link_slice_calls().load(); }
// corner_exchange_cand_kernel alone on a caller's configurations cfg [n][rows][cols] for the 2 x 3 / 3 x 2 window at (row1, col1):
// cand_out [n][2][4], flag_out [n][2], entry 0 LEFTUP_TO_RIGHTDOWN (kind 2), entry 1 LEFTDOWN_TO_RIGHTUP (kind 3)
int pepsgpu_diag_link_cand(int rows, int cols, int phys_dim, int n, const int32_t *cfg, int orient, int row1, int col1, int32_t *cand_out,
                           int32_t *flag_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(cfg && cand_out && flag_out, 1, "null buffer");
    PG_REQUIRE(orient == HORIZONTAL || orient == VERTICAL, 1, "bad orientation");
    PG_REQUIRE(rows >= 2 && cols >= 2 && phys_dim >= 1 && n >= 1 && (double)n * rows * cols < 2147483648.0, 1, "bad sizes");
    const int dr = orient == VERTICAL ? 2 : 1, dc = orient == VERTICAL ? 1 : 2;
    PG_REQUIRE(row1 >= 0 && row1 + dr < rows && col1 >= 0 && col1 + dc < cols, 1, "window outside the lattice");
    const int sites = rows * cols;
    const size_t ne = (size_t)n * sites;
    for (size_t e = 0; e < ne; ++e) PG_REQUIRE(cfg[e] >= 0 && cfg[e] < phys_dim, 1, "state outside [0, phys_dim)");
    DevBufs m;
    const int *dcfg = m.alloc<int>(ne, cfg);
    int *dc_ = m.alloc<int>(10 * (size_t)n), *df = dc_ + 8 * (size_t)n;
    const int s0 = row1 * cols + col1, s1 = s0 + dr * cols, s2 = s1 + dc, s3 = s0 + dc;   // upper-left, lower-left, lower-right, upper-right
    hipLaunchKernelGGL(corner_exchange_cand_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, 0, dcfg, sites, s0, s1, s2, s3, 2,
                       (int)LEFTUP_TO_RIGHTDOWN, (int)LEFTDOWN_TO_RIGHTUP, dc_, df, n);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(cand_out, dc_, 8 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(flag_out, df, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  });
}
int pepsgpu_walker_create(pepsgpu_ctx *ctx, int pos, int level, int *walker_out) {
  CTX_CALL(check_pos(pos); PG_REQUIRE(walker_out != nullptr, 1, "null output"); *walker_out = ctx->eng->walker_create(pos, level));
}
int pepsgpu_walker_clone(pepsgpu_ctx *ctx, int walker, int *walker_out) {
  CTX_CALL(PG_REQUIRE(walker_out != nullptr, 1, "null output"); *walker_out = ctx->eng->walker_clone(walker));
}
int pepsgpu_walker_destroy(pepsgpu_ctx *ctx, int walker) { CTX_CALL(ctx->eng->walker_destroy(walker)); }
int pepsgpu_walker_info(pepsgpu_ctx *ctx, int walker, int *pos_out, int *stack_size_out, int *bten_left_col_out, int *bten_right_col_out) {
  CTX_CALL(ctx->eng->walker_info(walker, pos_out, stack_size_out, bten_left_col_out, bten_right_col_out));
}
int pepsgpu_walker_set_mpo(pepsgpu_ctx *ctx, int walker, int num, const int32_t *states, const double *tensors, int n_tensors) {
  CTX_CALL(ctx->eng->walker_set_mpo(walker, num, states, tensors, n_tensors));
}
// structure_factor_measurement_mixin.h:127-134: the excited row, built on the device from the walkers' configuration table
int pepsgpu_walker_set_mpo_excited(pepsgpu_ctx *ctx, int walker, int num, int col, const int32_t *state_map, uint8_t *open_out) {
  CTX_CALL(ctx->eng->walker_set_mpo_excited(walker, num, col, state_map, open_out));
}
// structure_factor_measurement_mixin.h:160-194: the scan of one target row
int pepsgpu_walker_trace_slice(pepsgpu_ctx *ctx, int walker, int opp_level, const int32_t *site_map, const uint8_t *walker_mask, double *out) {
  CTX_CALL(ctx->eng->walker_trace_slice(walker, opp_level, site_map, walker_mask, out));
}
long pepsgpu_diag_walker_slice_calls(void) { return pepsgpu::walker_slice_calls().load(); }
// singlet_pair_correlation_measurement_mixin.h:376-401: the row of the reference bond with the pair injected, patched on the device
int pepsgpu_walker_set_mpo_excited_pair(pepsgpu_ctx *ctx, int walker, int num, int col, int d, const int32_t *occ, const int32_t *pair_table,
                                        int slot, uint8_t *open_out, int32_t *sign_out) {
  CTX_CALL(ctx->eng->walker_set_mpo_excited_pair(walker, num, col, d, occ, pair_table, slot, open_out, sign_out));
}
// :446-519: the two-site traces of one target row
int pepsgpu_walker_pair_trace_slice(pepsgpu_ctx *ctx, int walker, int opp_level, int d, const int32_t *occ, const int32_t *pair_table,
                                    const uint8_t *walker_mask, double *out) {
  CTX_CALL(ctx->eng->walker_pair_trace_slice(walker, opp_level, d, occ, pair_table, walker_mask, out));
}
long pepsgpu_diag_walker_pair_slice_calls(void) { return pepsgpu::walker_pair_slice_calls().load(); }
// walker_pair_cand_kernel and walker_excite_pair_kernel alone on a caller's extended rows ext [n][cols] (row-major variants 0 / 1) for
// the pair (col, col + 1): cand_out [n][2][2], skip_out [2][n], sign_out [n][2]; patched_out [n][cols] = the rows after the patch of `slot`
int pepsgpu_diag_walker_pair_cand(int cols, int d, const int32_t *occ, const int32_t *pair_table, int n, const int32_t *ext, int col,
                                  int slot, const uint8_t *walker_mask, int32_t *cand_out, int32_t *skip_out, int32_t *sign_out,
                                  int32_t *patched_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(ext && cand_out && skip_out && sign_out && patched_out, 1, "null buffer");
    PG_REQUIRE(cols >= 2 && n >= 1 && (double)n * cols < 2147483648.0, 1, "bad sizes");
    PG_REQUIRE(col >= 0 && col + 1 < cols, 1, "the pair is outside the row");
    PG_REQUIRE(slot == 0 || slot == 1, 1, "pair slot outside {0, 1}");
    pepsgpu::WalkerPairMap maps[2] = {};
    const unsigned occ_bits = pepsgpu::walker_pair_maps(d, 4 * d, occ, pair_table, &maps[0], &maps[1]);
    const size_t ne = (size_t)n * cols;
    for (size_t e = 0; e < ne; ++e) PG_REQUIRE(ext[e] >= 0 && ext[e] < 2 * d, 1, "extended state outside [0, 2 d)");
    std::vector<int> hmask;
    if (walker_mask) hmask.assign(walker_mask, walker_mask + n);
    DevBufs m;
    int *dtab = m.alloc<int>(ne, ext);
    const int *dmask = walker_mask ? m.alloc<int>((size_t)n, hmask.data()) : nullptr;
    int *dc = m.alloc<int>(8 * (size_t)n), *dk = dc + 4 * (size_t)n, *ds = dk + 2 * (size_t)n;
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(pepsgpu::walker_pair_cand_kernel, grid, block, 0, 0, (const int *)dtab, cols, col, d, occ_bits, maps[0], maps[1],
                       dmask, dc, dk, ds, n);
    PG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pepsgpu::walker_excite_pair_kernel, grid, block, 0, 0, dtab, cols, col, d, occ_bits, maps[slot], n);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(cand_out, dc, 4 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(skip_out, dk, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(sign_out, ds, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(patched_out, dtab, ne * sizeof(int), hipMemcpyDeviceToHost));
  });
}
int pepsgpu_walker_evolve(pepsgpu_ctx *ctx, int walker) { CTX_CALL(ctx->eng->walker_evolve(walker)); }
int pepsgpu_walker_evolve_step(pepsgpu_ctx *ctx, int walker) { CTX_CALL(ctx->eng->walker_evolve_step(walker)); }
int pepsgpu_walker_contract_row(pepsgpu_ctx *ctx, int walker, int opp_level, double *out) {
  CTX_CALL(PG_REQUIRE(out != nullptr, 1, "null output"); ctx->eng->walker_contract_row(walker, opp_level, out));
}
int pepsgpu_walker_init_bten(pepsgpu_ctx *ctx, int walker, int opp_level, int position, int target_col) {
  CTX_CALL(ctx->eng->walker_init_bten(walker, opp_level, position, target_col));
}
int pepsgpu_walker_grow_bten_step(pepsgpu_ctx *ctx, int walker, int opp_level, int position) {
  CTX_CALL(ctx->eng->walker_grow_bten_step(walker, opp_level, position));
}
int pepsgpu_walker_shift_bten_window(pepsgpu_ctx *ctx, int walker, int opp_level, int position) {
  CTX_CALL(ctx->eng->walker_shift_bten_window(walker, opp_level, position));
}
int pepsgpu_walker_trace_with_bten(pepsgpu_ctx *ctx, int walker, int opp_level, int site_col, int two_site, const int32_t *site_states,
                                   const double *site_tensors, int n_tensors, double *out) {
  CTX_CALL(PG_REQUIRE(out != nullptr, 1, "null output");
           PG_REQUIRE(!(site_states && site_tensors), 1, "name the replacement by states OR by tensors");
           ctx->eng->walker_trace(walker, opp_level, site_col, two_site, site_states, site_tensors, n_tensors, out));
}
int pepsgpu_walker_clear_bten(pepsgpu_ctx *ctx, int walker) { CTX_CALL(ctx->eng->walker_clear_bten(walker)); }
int pepsgpu_walker_get_bmps_tensor(pepsgpu_ctx *ctx, int walker, int idx, int *dims_out, double *data_out, double *logscale_out) {
  CTX_CALL(PG_REQUIRE(dims_out != nullptr, 1, "null dims"); ctx->eng->walker_get_tensor(walker, idx, dims_out, data_out, logscale_out));
}
int pepsgpu_bmps_park(pepsgpu_ctx *ctx, int pos, int keep_levels) { CTX_CALL(check_pos(pos); ctx->eng->bmps_park(pos, keep_levels)); }
int pepsgpu_bmps_unpark(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->bmps_unpark(pos)); }
int pepsgpu_generate_bmps_approach(pepsgpu_ctx *ctx, int pos) {
  CTX_CALL(check_pos(pos); ctx->eng->generate_bmps_approach(pos));
}
int pepsgpu_bmps_stack_size(pepsgpu_ctx *ctx, int pos) {
  if (!ctx || !ctx->eng || pos < 0 || pos > 3) return -1;
  return ctx->eng->bmps_size(pos);
}
int pepsgpu_bten_stack_size(pepsgpu_ctx *ctx, int pos) {
  if (!ctx || !ctx->eng || pos < 0 || pos > 3) return -1;
  return ctx->eng->bten_size(pos);
}
int pepsgpu_get_bmps_tensor(pepsgpu_ctx *ctx, int pos, int level, int idx, int *dims, double *data, double *ls) {
  CTX_CALL(check_pos(pos); ctx->eng->get_bmps_tensor(pos, level, idx, dims, data, ls));
}

int pepsgpu_init_bten(pepsgpu_ctx *ctx, int pos, int slice) { CTX_CALL(check_pos(pos); ctx->eng->init_bten(pos, slice)); }
int pepsgpu_grow_full_bten(pepsgpu_ctx *ctx, int pos, int slice, int remain, int init) {
  CTX_CALL(check_pos(pos); ctx->eng->grow_full_bten(pos, slice, remain, init));
}
int pepsgpu_grow_bten_step(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->grow_bten_step(pos)); }
int pepsgpu_shift_bten_window(pepsgpu_ctx *ctx, int pos) { CTX_CALL(check_pos(pos); ctx->eng->shift_bten_window(pos)); }
int pepsgpu_truncate_bten(pepsgpu_ctx *ctx, int pos, int len) { CTX_CALL(check_pos(pos); ctx->eng->truncate_bten(pos, len)); }

int pepsgpu_trace(pepsgpu_ctx *ctx, int row, int col, int dir, double *out) {
  CTX_CALL(ctx->eng->trace(row, col, dir, out));
}
int pepsgpu_replace_nn_trace(pepsgpu_ctx *ctx, int row, int col, int dir, int ncand, const int32_t *cand, double *out) {
  CTX_CALL(PG_REQUIRE(ncand >= 1 && cand, 1, "need >= 1 candidate"); ctx->eng->replace_nn_trace(row, col, dir, ncand, cand, out));
}
int pepsgpu_replace_one_trace(pepsgpu_ctx *ctx, int row, int col, int orient, int ncand, const int32_t *cand, double *out) {
  CTX_CALL(PG_REQUIRE(ncand >= 1 && cand, 1, "need >= 1 candidate"); ctx->eng->replace_one_trace(row, col, orient, ncand, cand, out));
}
int pepsgpu_init_bten2(pepsgpu_ctx *ctx, int pos, int slice) { CTX_CALL(check_pos(pos); ctx->eng->init_bten2(pos, slice)); }
int pepsgpu_grow_full_bten2(pepsgpu_ctx *ctx, int pos, int slice, int remain, int init) {
  CTX_CALL(check_pos(pos); ctx->eng->grow_full_bten2(pos, slice, remain, init));
}
int pepsgpu_grow_bten2_step(pepsgpu_ctx *ctx, int pos, int slice) {
  CTX_CALL(check_pos(pos); ctx->eng->grow_bten2_step(pos, slice));
}
int pepsgpu_shift_bten2_window(pepsgpu_ctx *ctx, int pos, int slice) {
  CTX_CALL(check_pos(pos); ctx->eng->shift_bten2_window(pos, slice));
}
int pepsgpu_bten2_stack_size(pepsgpu_ctx *ctx, int pos) {
  if (!ctx || !ctx->eng || pos < 0 || pos > 3) return -1;
  return ctx->eng->bten2_size(pos);
}
int pepsgpu_bten2_select_set(pepsgpu_ctx *ctx, int set) { CTX_CALL(ctx->eng->bten2_select_set(set)); }
int pepsgpu_cfg_override_slice(pepsgpu_ctx *ctx, int orient, int num, const int32_t *states) {
  CTX_CALL(ctx->eng->cfg_override_slice(orient, num, states));
}
int pepsgpu_replace_plaquette_trace(pepsgpu_ctx *ctx, int row, int col, int ncand, const int32_t *cand, int left_set, int right_set,
                                    double *out) {
  CTX_CALL(PG_REQUIRE(out && (ncand == 0 || cand), 1, "null argument");
           ctx->eng->replace_plaquette_trace(row, col, ncand, cand, left_set, right_set, out));
}
int pepsgpu_replace_nnn_trace(pepsgpu_ctx *ctx, int row, int col, int nnn_dir, int orient, int ncand, const int32_t *cand,
                              double *out) {
  CTX_CALL(PG_REQUIRE((ncand == 0 || cand) && ncand >= 0 && out, 1, "bad candidate table");
           PG_REQUIRE(nnn_dir == 0 || nnn_dir == 1, 1, "bad diagonal direction");
           ctx->eng->replace_nnn_trace(row, col, nnn_dir, orient, ncand, cand, out));
}
int pepsgpu_replace_tnn_trace(pepsgpu_ctx *ctx, int row, int col, int orient, int ncand, const int32_t *cand, double *out) {
  CTX_CALL(PG_REQUIRE((ncand == 0 || cand) && ncand >= 0 && out, 1, "bad candidate table");
           ctx->eng->replace_tnn_trace(row, col, orient, ncand, cand, out));
}
int pepsgpu_replace_sqrt5_trace(pepsgpu_ctx *ctx, int row, int col, int link_dir, int orient, int ncand,
                                const int32_t *cand, double *out) {
  CTX_CALL(PG_REQUIRE((ncand == 0 || cand) && ncand >= 0 && out, 1, "bad candidate table");
           PG_REQUIRE(link_dir == 0 || link_dir == 1, 1, "bad diagonal direction");
           ctx->eng->replace_sqrt5_trace(row, col, link_dir, orient, ncand, cand, out));
}
int pepsgpu_trace_scaling(pepsgpu_ctx *ctx, int on_device) {
  CTX_CALL(ctx->eng->trace_scaling_on_device = on_device != 0);
}
int pepsgpu_punch_hole(pepsgpu_ctx *ctx, int row, int col, int orient, double *out) {
  CTX_CALL(ctx->eng->punch_hole(row, col, orient, out));
}
int pepsgpu_grad_reset(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->grad_reset()); }
int pepsgpu_grad_accumulate_states(pepsgpu_ctx *ctx, const double *psi, const double *eloc, int exact_sum, const int32_t *states) {
  CTX_CALL(PG_REQUIRE(psi && eloc, 1, "null psi / eloc"); ctx->eng->grad_accumulate(psi, eloc, exact_sum, states));
}
int pepsgpu_grad_accumulate(pepsgpu_ctx *ctx, const double *psi, const double *eloc, int exact_sum) {
  CTX_CALL(PG_REQUIRE(psi && eloc, 1, "null psi / eloc"); ctx->eng->grad_accumulate(psi, eloc, exact_sum));
}
int pepsgpu_grad_read(pepsgpu_ctx *ctx, double *so, double *seo) {
  CTX_CALL(PG_REQUIRE(so && seo, 1, "null output"); ctx->eng->grad_read(so, seo));
}
int pepsgpu_grad_device_ptr(pepsgpu_ctx *ctx, void **so, void **seo, long *n_elems) {
  CTX_CALL(PG_REQUIRE(so && seo && n_elems, 1, "null output"); ctx->eng->grad_device_ptr(so, seo, n_elems));
}
int pepsgpu_comm_unique_id(void *id128_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(id128_out != nullptr, 1, "null output");
    ncclUniqueId id;
    PG_CHECK_RCCL(RcclApi::get().GetUniqueId(&id));
    memcpy(id128_out, &id, sizeof(id));
  });
}
int pepsgpu_comm_init(pepsgpu_ctx *ctx, int nranks, int rank, const void *id128) {
  CTX_CALL(ctx->comm.init(nranks, rank, id128));
}
int pepsgpu_comm_size(pepsgpu_ctx *ctx) { return ctx ? ctx->comm.nranks : -1; }
int pepsgpu_comm_rank(pepsgpu_ctx *ctx) { return ctx ? ctx->comm.rank : -1; }
int pepsgpu_comm_destroy(pepsgpu_ctx *ctx) { CTX_CALL(ctx->comm.destroy()); }
int pepsgpu_allreduce(pepsgpu_ctx *ctx, void *buf, long n, int dtype, int op, int on_device) {
  CTX_CALL(PG_REQUIRE(buf != nullptr || n == 0, 1, "null buffer"); PG_REQUIRE(n >= 0, 1, "negative count");
           ctx->comm.allreduce((hipStream_t)ctx->eng->stream_handle(), buf, (size_t)n, dtype, op, on_device != 0);
           if (on_device) ctx->eng->sync());
}
int pepsgpu_bcast_state(pepsgpu_ctx *ctx, int root) {
  CTX_CALL(void *p = nullptr; size_t bytes = 0; ctx->eng->state_device_ptr(&p, &bytes);
           PG_REQUIRE(ctx->comm.nranks == 1 || ctx->comm.comm != nullptr, 3, "pepsgpu_bcast_state: no communicator (pepsgpu_comm_init)");
           ctx->comm.bcast((hipStream_t)ctx->eng->stream_handle(), p, bytes, root);
           ctx->eng->state_adopted());
}
int pepsgpu_grad_allreduce(pepsgpu_ctx *ctx) {
  CTX_CALL(void *so = nullptr; void *seo = nullptr; long n = 0; ctx->eng->grad_device_ptr(&so, &seo, &n);
           hipStream_t s = (hipStream_t)ctx->eng->stream_handle();
           ctx->comm.allreduce(s, so, (size_t)n, 1, 0, true); ctx->comm.allreduce(s, seo, (size_t)n, 1, 0, true);
           ctx->eng->sync());
}
int pepsgpu_sr_begin(pepsgpu_ctx *ctx, int max_samples) { CTX_CALL(ctx->eng->sr_begin(max_samples)); }
int pepsgpu_sr_append(pepsgpu_ctx *ctx, const double *psi) { CTX_CALL(PG_REQUIRE(psi, 1, "null psi"); ctx->eng->sr_append(psi)); }
int pepsgpu_sr_count(pepsgpu_ctx *ctx) { return (ctx && ctx->eng) ? ctx->eng->sr_count() : -1; }
int pepsgpu_sr_sum(pepsgpu_ctx *ctx, double *out) { CTX_CALL(PG_REQUIRE(out, 1, "null output"); ctx->eng->sr_sum(out)); }
int pepsgpu_sr_matvec_c128(pepsgpu_ctx *ctx, const double *v, double mean_dot_v_re, double mean_dot_v_im, double scale, double *out) {
  CTX_CALL(PG_REQUIRE(v && out, 1, "null vector"); ctx->eng->sr_matvec(v, mean_dot_v_re, mean_dot_v_im, scale, out));
}
int pepsgpu_sr_matvec(pepsgpu_ctx *ctx, const double *v, double mean_dot_v, double scale, double *out) {
  CTX_CALL(PG_REQUIRE(v && out, 1, "null vector"); ctx->eng->sr_matvec(v, mean_dot_v, 0.0, scale, out));
}
int pepsgpu_sr_cg_solve(pepsgpu_ctx *ctx, const double *b, const double *x0, double diag_shift, int max_iter,
                        double relative_tolerance, double absolute_tolerance, int residual_recompute_interval,
                        double orthogonality_threshold, double *x_out, double *residual_norm, int *iterations, int *reason) {
  CTX_CALL(PG_REQUIRE(b && x_out && residual_norm && iterations && reason, 1, "null argument");
           PG_REQUIRE(max_iter >= 0 && relative_tolerance >= 0.0 && absolute_tolerance >= 0.0, 1, "bad CG parameters");
           ctx->eng->sr_cg_solve(b, x0, diag_shift, max_iter, relative_tolerance, absolute_tolerance, residual_recompute_interval,
                                 orthogonality_threshold, x_out, residual_norm, iterations, reason));
}
int pepsgpu_sr_gram(pepsgpu_ctx *ctx, const void *remote_samples_dev, const int32_t *remote_configs_dev, int n_remote, double *out) {
  CTX_CALL(PG_REQUIRE(out, 1, "null output"); ctx->eng->sr_gram(remote_samples_dev, remote_configs_dev, n_remote, out));
}
int pepsgpu_sr_weighted_sum(pepsgpu_ctx *ctx, const double *y, double *out) {
  CTX_CALL(PG_REQUIRE(y && out, 1, "null argument"); ctx->eng->sr_weighted_sum(y, out));
}
int pepsgpu_sr_copy_samples(pepsgpu_ctx *ctx, void *dst_samples_dev, int32_t *dst_configs_dev) {
  CTX_CALL(PG_REQUIRE(dst_samples_dev && dst_configs_dev, 1, "null destination"); ctx->eng->sr_copy_samples(dst_samples_dev, dst_configs_dev));
}
// ---- device-resident optimisation step (engine_opt.h) ----
int pepsgpu_opt_begin(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->opt_begin()); }
int pepsgpu_opt_end(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->opt_end()); }
int pepsgpu_opt_gradient_from_accumulators(pepsgpu_ctx *ctx, const double *e_loc_sum, double weight_sum, double *energy_out,
                                           double *grad_norm_out) {
  CTX_CALL(PG_REQUIRE(e_loc_sum != nullptr, 1, "null e_loc_sum");
           ctx->eng->opt_gradient_from_accumulators(e_loc_sum, weight_sum, energy_out, grad_norm_out));
}
int pepsgpu_opt_set_gradient(pepsgpu_ctx *ctx, const double *host) {
  CTX_CALL(PG_REQUIRE(host != nullptr, 1, "null gradient"); ctx->eng->opt_set_gradient(host));
}
int pepsgpu_opt_get_gradient(pepsgpu_ctx *ctx, double *host) {
  CTX_CALL(PG_REQUIRE(host != nullptr, 1, "null output"); ctx->eng->opt_get_gradient(host));
}
int pepsgpu_opt_clip(pepsgpu_ctx *ctx, double clip_value, double clip_norm, double *norm_before_out) {
  CTX_CALL(ctx->eng->opt_clip(clip_value, clip_norm, norm_before_out));
}
int pepsgpu_opt_natural_gradient(pepsgpu_ctx *ctx, double diag_shift, int max_iter, double relative_tolerance, double absolute_tolerance,
                                 int residual_recompute_interval, double orthogonality_threshold, double *residual_norm, int *iterations,
                                 int *reason, double *direction_norm_out) {
  CTX_CALL(PG_REQUIRE(residual_norm && iterations && reason, 1, "null argument");
           PG_REQUIRE(max_iter >= 0 && relative_tolerance >= 0.0 && absolute_tolerance >= 0.0, 1, "bad CG parameters");
           ctx->eng->opt_natural_gradient(diag_shift, max_iter, relative_tolerance, absolute_tolerance, residual_recompute_interval,
                                          orthogonality_threshold, residual_norm, iterations, reason, direction_norm_out));
}
int pepsgpu_opt_step(pepsgpu_ctx *ctx, int rule, double lr, const double *params, int n_params) {
  CTX_CALL(ctx->eng->opt_step(rule, lr, params, n_params));
}
int pepsgpu_opt_scale_state(pepsgpu_ctx *ctx, double factor) { CTX_CALL(ctx->eng->opt_scale_state(factor)); }
int pepsgpu_opt_read_state(pepsgpu_ctx *ctx, double *host) {
  CTX_CALL(PG_REQUIRE(host != nullptr, 1, "null output"); ctx->eng->opt_read_state(host));
}
// ---- the lowest-energy parameters of a VMC run, kept in HBM (engine_opt.h) ----
int pepsgpu_vmc_snapshot_save(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->vmc_snapshot_save()); }
int pepsgpu_vmc_snapshot_read(pepsgpu_ctx *ctx, double *host) {
  CTX_CALL(PG_REQUIRE(host != nullptr, 1, "null output"); ctx->eng->vmc_snapshot_read(host));
}
int pepsgpu_vmc_snapshot_clear(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->vmc_snapshot_clear()); }
// ---- the base of a step: rollback and step-selector trials in HBM (engine_guard.h) ----
int pepsgpu_guard_base_save(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->opt_base_save()); }
int pepsgpu_guard_base_restore(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->opt_base_restore()); }
int pepsgpu_guard_base_clear(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->opt_base_clear()); }
int pepsgpu_guard_preview(pepsgpu_ctx *ctx, int rule, double lr, const double *params, int n_params) {
  CTX_CALL(ctx->eng->opt_preview(rule, lr, params, n_params));
}
int pepsgpu_minsr_direction(pepsgpu_ctx *ctx, const double *eloc, const double *energy, double r_pinv, double a_pinv, int soft_cutoff,
                            double *direction_norm_out, double *info_out) {
  CTX_CALL(ctx->eng->minsr_direction(eloc, energy, r_pinv, a_pinv, soft_cutoff, direction_norm_out, info_out));
}
// ---- L-BFGS on the optimizer buffers (engine_lbfgs.h) ----
int pepsgpu_lbfgs_begin(pepsgpu_ctx *ctx, int history_size) { CTX_CALL(ctx->eng->lbfgs_begin(history_size)); }
int pepsgpu_lbfgs_end(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->lbfgs_end()); }
int pepsgpu_lbfgs_reset(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->lbfgs_reset()); }
int pepsgpu_lbfgs_update(pepsgpu_ctx *ctx, double min_curvature, int use_damping, int *outcome, double *curvature) {
  CTX_CALL(ctx->eng->lbfgs_update(min_curvature, use_damping, outcome, curvature));
}
int pepsgpu_lbfgs_direction(pepsgpu_ctx *ctx, double min_curvature, double max_direction_norm, double *dphi0, double *norm,
                            int *was_reset) {
  CTX_CALL(ctx->eng->lbfgs_direction(min_curvature, max_direction_norm, dphi0, norm, was_reset));
}
int pepsgpu_lbfgs_trial(pepsgpu_ctx *ctx, double alpha) { CTX_CALL(ctx->eng->lbfgs_trial(alpha)); }
int pepsgpu_lbfgs_slope(pepsgpu_ctx *ctx, double *dphi) {
  CTX_CALL(PG_REQUIRE(dphi != nullptr, 1, "null output"); ctx->eng->lbfgs_slope(dphi));
}
int pepsgpu_lbfgs_commit(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->lbfgs_commit()); }
int pepsgpu_lbfgs_get_direction(pepsgpu_ctx *ctx, double *out) {
  CTX_CALL(PG_REQUIRE(out != nullptr, 1, "null output"); ctx->eng->lbfgs_get_direction(out));
}
int pepsgpu_lbfgs_get_pair(pepsgpu_ctx *ctx, int index, double *s_out, double *y_out) {
  CTX_CALL(ctx->eng->lbfgs_get_pair(index, s_out, y_out));
}
int pepsgpu_lbfgs_counters(pepsgpu_ctx *ctx, long *out4) {
  CTX_CALL(PG_REQUIRE(out4 != nullptr, 1, "null output"); ctx->eng->lbfgs_counters(out4));
}
// the eigensolver of pepsgpu_minsr_direction alone, on the context's device and stream (eigh_jacobi.h)
int pepsgpu_diag_eigh(pepsgpu_ctx *ctx, int n, int is_complex, const double *a, double *w_out, double *z_out, int *sweeps_out) {
  CTX_CALL(diag_eigh_impl((hipStream_t)ctx->eng->stream_handle(), n, is_complex, a, w_out, z_out, sweeps_out));
}
int pepsgpu_fermion_decoration_set(pepsgpu_ctx *ctx, int d, const int32_t *nf, const uint8_t *bond_parity) {
  CTX_CALL(ctx->eng->fermion_decoration_set(d, nf, bond_parity));
}
int pepsgpu_update_local(pepsgpu_ctx *ctx, int nsites, const int32_t *sites, const int32_t *ns, const uint8_t *mask) {
  CTX_CALL(ctx->eng->update_local(nsites, sites, ns, mask));
}
int pepsgpu_erase_envs_after_update(pepsgpu_ctx *ctx, int row, int col) {
  CTX_CALL(ctx->eng->erase_envs_after_update(row, col));
}
int pepsgpu_evaluate_amplitude(pepsgpu_ctx *ctx, double *out) { CTX_CALL(ctx->eng->evaluate_amplitude(out)); }
int pepsgpu_walker_flags(pepsgpu_ctx *ctx, int32_t *out) { CTX_CALL(ctx->eng->read_flags(out)); }
int pepsgpu_sync(pepsgpu_ctx *ctx) { CTX_CALL(ctx->eng->sync()); }
int pepsgpu_stats(pepsgpu_ctx *ctx, double *out, int n) { CTX_CALL(ctx->eng->stats(out, n)); }
int pepsgpu_profile_enable(pepsgpu_ctx *ctx, int on) { CTX_CALL(ctx->eng->profile_enable(on)); }
int pepsgpu_profile_read(pepsgpu_ctx *ctx, double *out) { CTX_CALL(ctx->eng->profile_read(out)); }

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// diagnostics
template <typename TI, typename TO, typename TAcc>
static void diag_tgemm_t(const TGemmDesc &d, const void *A, size_t na, const void *B, size_t nb, void *C, size_t nc) {
  TI *dA, *dB;
  TO *dC;
  PG_CHECK_HIP(hipMalloc(&dA, na * sizeof(TI)));
  PG_CHECK_HIP(hipMalloc(&dB, nb * sizeof(TI)));
  PG_CHECK_HIP(hipMalloc(&dC, nc * sizeof(TO)));
  PG_CHECK_HIP(hipMemcpy(dA, A, na * sizeof(TI), hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemcpy(dB, B, nb * sizeof(TI), hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemcpy(dC, C, nc * sizeof(TO), hipMemcpyHostToDevice));
  tgemm_launch<TI, TI, TO, TAcc>(0, d, dA, dB, dC);
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(C, dC, nc * sizeof(TO), hipMemcpyDeviceToHost));
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
}

extern "C" int pepsgpu_diag_tgemm(int dtype_in, int dtype_out, const int *di, int n_ints, const void *A, size_t na, const void *B,
                       size_t nb, void *C, size_t nc, int nbatch, long wA, long wB, long wC) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(n_ints == 27, 1, "descriptor needs 27 ints");
    TGemmDesc d;
    for (int k = 0; k < 3; ++k) {
      d.I[k] = di[k]; d.J[k] = di[3 + k]; d.K[k] = di[6 + k];
      d.sAi[k] = di[9 + k]; d.sAk[k] = di[12 + k]; d.sBk[k] = di[15 + k];
      d.sBj[k] = di[18 + k]; d.sCi[k] = di[21 + k]; d.sCj[k] = di[24 + k];
    }
    d.wA = wA; d.wB = wB; d.wC = wC; d.nbatch = nbatch;
    // PEPSGPU_DIAG_TGEMM_MODE (read per call; f32 only): 1 = the wave-per-tile kernel (a per-entry live extent equal to the static one
    // routes there), 2 = the same with float64 accumulation on the f64 matrix cores (tg_direct_body_f64)
    const char *mode_s = getenv("PEPSGPU_DIAG_TGEMM_MODE");
    const int mode = mode_s ? atoi(mode_s) : 0;
    int *dext = nullptr;
    if (mode && dtype_in == 0 && dtype_out == 0) {
      std::vector<int> h(nbatch, d.I[2]);
      PG_CHECK_HIP(hipMalloc(&dext, sizeof(int) * nbatch));
      PG_CHECK_HIP(hipMemcpy(dext, h.data(), sizeof(int) * nbatch, hipMemcpyHostToDevice));
      d.dI[2].p = dext;
      d.acc64 = mode == 2;
    }
    struct Guard { int *p; ~Guard() { if (p) (void)hipFree(p); } } guard{dext};
    if (dtype_in == 0 && dtype_out == 0) diag_tgemm_t<float, float, float>(d, A, na, B, nb, C, nc);
    else if (dtype_in == 1 && dtype_out == 1) diag_tgemm_t<double, double, double>(d, A, na, B, nb, C, nc);
    else if (dtype_in == 0 && dtype_out == 1) diag_tgemm_t<float, double, double>(d, A, na, B, nb, C, nc);
    else throw Error(1, "unsupported dtype combination");
  });
}

// ---- the whole TGemmDesc from flat arrays (pepsgpu_diag_tgemm_desc / pepsgpu_diag_tgemm_route; layout in include/pepsgpu.h) ----
constexpr int TGD_NI = 89, TGD_NL = 5, TGD_ND = 1;
// pool: base of the per-batch int arrays the descriptor points into (an offset < 0 = null pointer); scale_in: the per-entry
// input scales (used when desc_ints[87] != 0)
static TGemmDesc tgd_unpack(const int *di, const long *dl, const double *dd, const int *pool, const float *scale_in) {
  TGemmDesc d;
  auto ptr = [&](int off) -> const int * { return off >= 0 ? pool + off : nullptr; };
  for (int k = 0; k < 3; ++k) {
    d.I[k] = di[k]; d.J[k] = di[3 + k]; d.K[k] = di[6 + k];
    d.sAi[k] = di[9 + k]; d.sAk[k] = di[12 + k]; d.sBk[k] = di[15 + k];
    d.sBj[k] = di[18 + k]; d.sCi[k] = di[21 + k]; d.sCj[k] = di[24 + k];
  }
  TgDyn *dyn[9] = {&d.dI[0], &d.dI[1], &d.dI[2], &d.dJ[0], &d.dJ[1], &d.dJ[2], &d.dK[0], &d.dK[1], &d.dK[2]};
  for (int q = 0; q < 9; ++q) {
    dyn[q]->p = ptr(di[27 + q]); dyn[q]->mul = di[36 + q]; dyn[q]->mask = di[45 + q]; dyn[q]->div = di[54 + q];
  }
  d.dynI = ptr(di[63]); d.dynK = ptr(di[64]); d.dynI_mul = di[65]; d.dynK_mul = di[66];
  d.selA = ptr(di[67]); d.selB = ptr(di[68]); d.selA_inc = di[69]; d.selB_inc = di[70];
  d.bdivA = di[71]; d.bdivB = di[72]; d.bdivC = di[73]; d.seldivA = di[74]; d.seldivB = di[75];
  d.nbatch = di[76]; d.accumulate = di[77]; d.upper_only = di[78]; d.conjA = di[79]; d.conjB = di[80];
  d.batch_flag = ptr(di[81]); d.prefer_tiled = di[82]; d.acc64 = di[83];
  d.scale_in = di[87] ? scale_in : nullptr;
  d.wA = dl[0]; d.wB = dl[1]; d.wC = dl[2]; d.selA_mul = dl[3]; d.selB_mul = dl[4];
  d.alpha = dd[0];
  return d;
}

static void tgd_check(int n_ints, int n_longs, int n_dbls) {
  PG_REQUIRE(n_ints == TGD_NI && n_longs == TGD_NL && n_dbls == TGD_ND, 1, "descriptor needs 89 ints, 5 longs, 1 double");
}

static void tgd_put_route(const TgRoute &r, int32_t *route_out) {
  route_out[0] = r.kind; route_out[1] = r.avec; route_out[2] = r.bvec; route_out[3] = r.acc64;
}

// the five element-type instantiations tgemm_launch is called with: (TA, TB, TC, TAcc)
template <typename F>
static void tgd_dispatch(int types, F &&f) {
  switch (types) {
    case 0: f((float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr); break;
    case 1: f((float *)nullptr, (float *)nullptr, (float *)nullptr, (double *)nullptr); break;
    case 2: f((float *)nullptr, (float *)nullptr, (double *)nullptr, (double *)nullptr); break;
    case 3: f((double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr); break;
    case 4: f((c128 *)nullptr, (c128 *)nullptr, (c128 *)nullptr, (c128 *)nullptr); break;
    default: throw Error(1, "unsupported element types");
  }
}

extern "C" int pepsgpu_diag_tgemm_route(int types, const int *desc_ints, int n_ints, const long *desc_longs, int n_longs,
                                        const double *desc_dbls, int n_dbls, long a_offset, long b_offset, int32_t *route_out) {
  return guarded(nullptr, [&]() {
    tgd_check(n_ints, n_longs, n_dbls);
    // no device access: the operand pointers are only tested for alignment (a buffer from hipMalloc, advanced by the offsets)
    static const int fake_pool[1] = {0};
    static const float fake_scale[1] = {1.f};
    static float fake_out[1];
    TGemmDesc d = tgd_unpack(desc_ints, desc_longs, desc_dbls, fake_pool, fake_scale);
    if (desc_ints[84]) d.scale_out = fake_out;
    tgd_dispatch(types, [&](auto *ta, auto *tb, auto *tc, auto *tacc) {
      using TA = std::remove_pointer_t<decltype(ta)>; using TB = std::remove_pointer_t<decltype(tb)>;
      using TC = std::remove_pointer_t<decltype(tc)>; using TAcc = std::remove_pointer_t<decltype(tacc)>;
      (void)tc; (void)tacc;
      const TA *A = (const TA *)(uintptr_t)4096 + a_offset;
      const TB *B = (const TB *)(uintptr_t)4096 + b_offset;
      tgd_put_route(tgemm_route<TA, TB, TC, TAcc>(d, A, B), route_out);
    });
  });
}

extern "C" int pepsgpu_diag_tgemm_desc(int types, const int *desc_ints, int n_ints, const long *desc_longs, int n_longs,
                                       const double *desc_dbls, int n_dbls, const int32_t *pool, long pool_n, const float *scale_in,
                                       const void *A, size_t a_elems, long a_offset, const void *B, size_t b_elems, long b_offset,
                                       void *C, size_t c_elems, float *scale_out, double *norm_log, int32_t *norm_flag,
                                       int32_t *route_out, unsigned long long *flops_out) {
  unsigned long long *const saved_flop = tg_flop_counter, *const saved_byte = tg_byte_counter;
  const int rc = guarded(nullptr, [&]() {
    tgd_check(n_ints, n_longs, n_dbls);
    PG_REQUIRE(a_offset >= 0 && (size_t)a_offset <= a_elems && b_offset >= 0 && (size_t)b_offset <= b_elems, 1, "operand offset outside its buffer");
    const int nbatch = desc_ints[76];
    DevBufs m;
    const int *dpool = m.alloc<int>(pool_n > 0 ? (size_t)pool_n : 0, pool);
    const float *dscale_in = desc_ints[87] ? m.alloc<float>(std::max(nbatch, 0), scale_in) : nullptr;
    TGemmDesc d = tgd_unpack(desc_ints, desc_longs, desc_dbls, dpool, dscale_in);
    float *dso = nullptr;
    double *dnl = nullptr;
    int *dnf = nullptr;
    if (desc_ints[84]) d.scale_out = dso = m.alloc<float>(std::max(nbatch, 0), scale_out);
    if (desc_ints[85]) d.norm_log = dnl = m.alloc<double>(std::max(nbatch, 0), norm_log);
    if (desc_ints[86]) d.norm_flag = dnf = m.alloc<int>(std::max(nbatch, 0), norm_flag);
    unsigned long long *dflop = m.alloc<unsigned long long>(1);
    PG_CHECK_HIP(hipMemset(dflop, 0, sizeof(unsigned long long)));
    tgd_dispatch(types, [&](auto *ta, auto *tb, auto *tc, auto *tacc) {
      using TA = std::remove_pointer_t<decltype(ta)>; using TB = std::remove_pointer_t<decltype(tb)>;
      using TC = std::remove_pointer_t<decltype(tc)>; using TAcc = std::remove_pointer_t<decltype(tacc)>;
      (void)tacc;
      const TA *dA = m.alloc<TA>(a_elems, A) + a_offset;
      const TB *dB = m.alloc<TB>(b_elems, B) + b_offset;
      TC *dC = m.alloc<TC>(c_elems, C);
      tgd_put_route(tgemm_route<TA, TB, TC, TAcc>(d, dA, dB), route_out);
      tg_flop_counter = dflop;
      tg_byte_counter = nullptr;
      tgemm_launch<TA, TB, TC, TAcc>(0, d, dA, dB, dC);
      PG_CHECK_HIP(hipDeviceSynchronize());
      PG_CHECK_HIP(hipMemcpy(C, dC, c_elems * sizeof(TC), hipMemcpyDeviceToHost));
      (void)tc;
    });
    if (dso) PG_CHECK_HIP(hipMemcpy(scale_out, dso, nbatch * sizeof(float), hipMemcpyDeviceToHost));
    if (dnl) PG_CHECK_HIP(hipMemcpy(norm_log, dnl, nbatch * sizeof(double), hipMemcpyDeviceToHost));
    if (dnf) PG_CHECK_HIP(hipMemcpy(norm_flag, dnf, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(flops_out, dflop, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  });
  tg_flop_counter = saved_flop;
  tg_byte_counter = saved_byte;
  return rc;
}

// One BTen growth step through tgemm_chain3_kernel with the descriptors of Engine::bten_step (bten_chain_descs):
//   out[b][x,s2,y] = sum mps1[b][x,p1,c] bten[b][c,b1,b2] site[sel[b*sel_inc]][p1,b1,s1,s2] mps2[b][b2,s1,y]
// dims8 = {x, p1, cdim, b1, b2, s1, s2, y}; site_strides4 = element strides of the site legs (p1, b1, s1, s2), one tensor per
// slot of `slot` elements, nslots of them; live4 (nullable) = per entry {vx, vc, vb, vy}; skip (nullable) = per entry;
// offs3 = element offsets of the mps1 / bten / site bases in their buffers (alignment variants).  out holds the initial
// contents (entries the kernel does not write keep them).  launched_out = the launcher's return (0: shapes declined, nothing
// launched; 2: launched), flags_out[b] = the kernel's flag, variant_out = {avec1, bvec1, avec2}.
extern "C" int pepsgpu_diag_tgemm_chain3(const int *dims8, const int *site_strides4, long slot, int nslots, const int32_t *sel, int sel_inc,
                                         const int32_t *live4, const int32_t *skip, int nbatch, const int *offs3, const float *mps1,
                                         const float *bten, const float *site, const float *mps2, float *out, int32_t *flags_out,
                                         int32_t *launched_out, int32_t *variant_out) {
  return guarded(nullptr, [&]() {
    const int x = dims8[0], p1 = dims8[1], cdim = dims8[2], b1 = dims8[3], b2 = dims8[4], s1 = dims8[5], s2 = dims8[6], y = dims8[7];
    PG_REQUIRE(nbatch > 0 && nslots > 0 && sel_inc >= 0 && offs3[0] >= 0 && offs3[1] >= 0 && offs3[2] >= 0, 1, "bad arguments");
    const long n1 = (long)x * p1 * cdim, nbt = (long)cdim * b1 * b2, n2 = (long)b2 * s1 * y, no = (long)x * s2 * y;
    DevBufs m;
    const float *dm1 = m.alloc<float>(n1 * nbatch + offs3[0], mps1) + offs3[0];
    const float *dbt = m.alloc<float>(nbt * nbatch + offs3[1], bten) + offs3[1];
    const float *dsite = m.alloc<float>((size_t)slot * nslots + offs3[2], site) + offs3[2];
    const float *dm2 = m.alloc<float>(n2 * nbatch, mps2);
    float *dout = m.alloc<float>(no * nbatch, out);
    const int *dsel = m.alloc<int>((size_t)(nbatch - 1) * sel_inc + 1, sel);
    int *dflag = m.alloc<int>(nbatch, flags_out);
    const int *dskip = skip ? m.alloc<int>(nbatch, skip) : nullptr;
    const int *vl[4] = {nullptr, nullptr, nullptr, nullptr};
    if (live4) {
      std::vector<int> h(4 * (size_t)nbatch);     // [vx | vc | vb | vy] as four arrays
      for (int b = 0; b < nbatch; ++b)
        for (int q = 0; q < 4; ++q) h[(size_t)q * nbatch + b] = live4[4 * b + q];
      const int *dl = m.alloc<int>(h.size(), h.data());
      for (int q = 0; q < 4; ++q) vl[q] = dl + (size_t)q * nbatch;
    }
    const BTenChainDescs cd = bten_chain_descs(x, p1, cdim, b1, b2, s1, s2, y, site_strides4[0], site_strides4[1], site_strides4[2],
                                               site_strides4[3], n1, nbt, n2, dsel, sel_inc, slot, nbatch, vl[0], vl[1], vl[2], vl[3]);
    variant_out[0] = tg_vec_a(cd.g1, dm1); variant_out[1] = tg_vec_b(cd.g1, dbt); variant_out[2] = tg_vec_a(cd.g2, dsite);
    launched_out[0] = tgemm_chain3_launch(0, cd.g1, cd.g2, cd.g3, cd.mp, cd.mp3, dm1, dbt, dsite, dm2, dout, dflag, dskip);
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(out, dout, no * nbatch * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(flags_out, dflag, nbatch * sizeof(int), hipMemcpyDeviceToHost));
  });
}

// Forward pair of an absorption through tgemm_chain_kernel exactly as Engine::absorb_impl sets it up:
//   X[m,l,p,a2] = sum_a R[m,l,a] A[a,p,a2]  (kept in LDS),   P[m,u,l2,a2] = sum_{l,p} W[l,p,l2,u] X[m,l,p,a2]
// dims = {m, l, a, p, a2, l2, u} (static), live = per entry {m_live, a_live, a2_live}; W is one tensor per entry.
// flags_out[b] = 0 done, -1 the live X exceeds the LDS buffer (P[b] untouched).
extern "C" int pepsgpu_diag_tgemm_chain(const int *dims, const int32_t *live, int nbatch, const float *R, const float *A,
                                        const float *W, float *P_out, int32_t *flags_out) {
  return guarded(nullptr, [&]() {
    const int m = dims[0], l = dims[1], a = dims[2], p = dims[3], a2 = dims[4], l2 = dims[5], u = dims[6];
    const size_t nR = (size_t)m * l * a, nA = (size_t)a * p * a2, nW = (size_t)l * p * l2 * u, nP = (size_t)m * u * l2 * a2;
    float *dR, *dA, *dW, *dP;
    int *dl, *dflag;
    PG_CHECK_HIP(hipMalloc(&dR, nR * nbatch * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dA, nA * nbatch * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dW, nW * nbatch * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dP, nP * nbatch * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dl, 3 * (size_t)nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dflag, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dR, R, nR * nbatch * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dA, A, nA * nbatch * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dW, W, nW * nbatch * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dP, 0, nP * nbatch * sizeof(float)));
    std::vector<int> hl(3 * (size_t)nbatch);      // [m_live | a_live | a2_live] as three arrays
    for (int b = 0; b < nbatch; ++b)
      for (int q = 0; q < 3; ++q) hl[(size_t)q * nbatch + b] = live[3 * b + q];
    PG_CHECK_HIP(hipMemcpy(dl, hl.data(), hl.size() * sizeof(int), hipMemcpyHostToDevice));
    const int *ml = dl, *al = dl + nbatch, *a2l = dl + 2 * nbatch;
    TGemmDesc gx, gp;
    gx.I[1] = m; gx.I[2] = l; gx.sAi[1] = l * a; gx.sAi[2] = a; gx.sCi[1] = l * p * a2; gx.sCi[2] = p * a2;
    gx.K[2] = a; gx.sAk[2] = 1; gx.sBk[2] = p * a2;
    gx.J[1] = p; gx.J[2] = a2; gx.sBj[1] = a2; gx.sBj[2] = 1; gx.sCj[1] = a2; gx.sCj[2] = 1;
    gx.wA = (long)nR; gx.wB = (long)nA; gx.wC = 0; gx.nbatch = nbatch;
    gx.dI[1].p = ml; gx.dK[2].p = al; gx.dJ[2].p = a2l;
    gp.I[1] = l2; gp.I[2] = u; gp.sAi[1] = u; gp.sAi[2] = 1; gp.sCi[1] = a2; gp.sCi[2] = l2 * a2;
    gp.K[1] = l; gp.K[2] = p; gp.sAk[1] = p * l2 * u; gp.sAk[2] = l2 * u;
    gp.J[1] = m; gp.J[2] = a2; gp.sCj[1] = u * l2 * a2; gp.sCj[2] = 1;
    gp.wA = (long)nW; gp.wC = (long)nP; gp.nbatch = nbatch;
    gp.dJ[1].p = ml; gp.dJ[2].p = a2l;
    TGemmChainMap mp;
    mp.mapK[1] = 2; mp.mapK[2] = 4;
    mp.mapJ[1] = 1; mp.mapJ[2] = 5;
    const char *f64_s = getenv("PEPSGPU_DIAG_CHAIN_F64");      // (read per call) 1: the float64-accumulating form of both stages
    const char *tri_s = getenv("PEPSGPU_DIAG_TRI");            // (read per call) 1: R is a row-compacted triangular factor, its zero blocks are skipped
    PG_REQUIRE(tgemm_chain_launch(0, gx, gp, mp, dR, dA, dW, dP, dflag, 1, tri_s && atoi(tri_s) ? 1 : 0, f64_s && atoi(f64_s) ? 1 : 0,
                                  tri_s && atoi(tri_s) ? 1 : 0), 1, "chain launch refused");
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(P_out, dP, nP * nbatch * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(flags_out, dflag, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dR); (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dP); (void)hipFree(dl); (void)hipFree(dflag);
  });
}

// The forward pair (P = W (R A)) or the backward pair (Tt = W (A Y)) of an absorption through tgemm_chain_launch, with the
// descriptors of Engine::forward_pair / backward_pair (absorb_desc.h) and the site tensor reached through a selector table:
//   dims8 = {m, a, a2, k2, l, p, l2, u} (static); site_strides4 = element strides of the legs (l, p, l2, u) of one site tensor,
//   `nslots` tensors of `slot` elements in `site`, entry b uses tensor sel[b]
//   forward:  op1 = R [nbatch][m][l][a], op2 = A [nbatch][a][p][a2], live3 = per entry {m, a, a2}, out = P [nbatch][m][u][l2][a2]
//   backward: op1 = A [nbatch][a][p][a2], op2 = Y [nbatch][l2][a2][k2], live3 = per entry {a, a2, k2},
//             out = Tt [nbatch][l][a][u][k2] ([l][a][k2][u] with opts & 2); scale_in (nullable) = per-entry input scale
//   opts: 1 the leg-8 kernel where its contract holds (else tgemm_chain_kernel), 2 tsw, 4 the zero-filling (masked) k2 extent of
//         the first site, 8 the float64-accumulating form
// out holds the initial contents (what no kernel stores comes back unchanged).  flags_out[b] = the kernel's flag;
// info_out = {the launcher's return, 1 when the leg-8 kernel ran}.
extern "C" int pepsgpu_diag_tgemm_chain_pair(int backward, const int *dims8, const int *site_strides4, long slot, int nslots,
                                             const int32_t *sel, const int32_t *live3, int nbatch, int opts, const float *scale_in,
                                             const float *op1, const float *op2, const float *site, float *out, int32_t *flags_out,
                                             int32_t *info_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(nbatch > 0 && nslots > 0 && slot > 0 && dims8 && site_strides4 && sel && live3 && op1 && op2 && site && out, 1, "bad arguments");
    SiteDims d;
    d.m = dims8[0]; d.a = dims8[1]; d.a2 = dims8[2]; d.k2 = dims8[3]; d.l = dims8[4]; d.p = dims8[5]; d.l2 = dims8[6]; d.u = dims8[7];
    d.ll = 0; d.lp = 1; d.lr = 2; d.lu = 3;
    for (int q = 0; q < 4; ++q) d.st[q] = site_strides4[q];
    d.la = d.l * d.a; d.uk = d.u * d.k2;
    for (int b = 0; b < nbatch; ++b) PG_REQUIRE(sel[b] >= 0 && sel[b] < nslots, 1, "selector beyond the site store");
    const long n1 = backward ? (long)d.a * d.p * d.a2 : (long)d.m * d.l * d.a;
    const long n2 = backward ? (long)d.l2 * d.a2 * d.k2 : (long)d.a * d.p * d.a2;
    const long no = backward ? (long)d.l * d.a * d.u * d.k2 : (long)d.m * d.u * d.l2 * d.a2;
    DevBufs mb;
    const float *d1p = mb.alloc<float>(n1 * nbatch, op1), *d2p = mb.alloc<float>(n2 * nbatch, op2);
    const float *dsite = mb.alloc<float>((size_t)slot * nslots, site);
    float *dout = mb.alloc<float>(no * nbatch, out);
    const int *dsel = mb.alloc<int>(nbatch, sel);
    const float *dscale = scale_in ? mb.alloc<float>(nbatch, scale_in) : nullptr;
    int *dflag = mb.alloc<int>(nbatch, flags_out);
    std::vector<int> hl(3 * (size_t)nbatch);
    for (int b = 0; b < nbatch; ++b)
      for (int q = 0; q < 3; ++q) hl[(size_t)q * nbatch + b] = live3[3 * b + q];
    const int *dl = mb.alloc<int>(hl.size(), hl.data());
    const int *v0 = dl, *v1 = dl + nbatch, *v2 = dl + 2 * (size_t)nbatch;
    TGemmDesc g1, g2;
    if (backward) {
      g1 = desc_z1(d, n1, n2, 0, nbatch, v0, v1, v2);
      g1.scale_in = dscale;
      g2 = desc_tt(d, (opts & 2) != 0, 0, no, nbatch, v0, v2, (opts & 4) != 0);
    } else {
      g1 = desc_x(d, n1, n2, 0, nbatch, v0, 1, v1, v2);
      g2 = desc_p(d, 0, no, nbatch, v0, 1, v2);
    }
    g2.selA = dsel; g2.selA_mul = slot; g2.selA_inc = 1; g2.seldivA = 1; g2.wA = 0;
    TGemmChainMap mp;
    mp.mapK[1] = 2; mp.mapK[2] = 4;
    mp.mapJ[1] = 1; mp.mapJ[2] = 5;
    const long before = tg_chain_d8_count.load();
    tg_chain_d8_force = (opts & 1) ? 1 : 0;
    int rc = 0;
    try {
      rc = tgemm_chain_launch(0, g1, g2, mp, d1p, d2p, dsite, dout, dflag, 1, 0, (opts & 8) ? 1 : 0);
    } catch (...) { tg_chain_d8_force = -1; throw; }
    tg_chain_d8_force = -1;
    PG_REQUIRE(rc != 0, 1, "chain launch refused");
    PG_CHECK_HIP(hipDeviceSynchronize());
    info_out[0] = rc;
    info_out[1] = tg_chain_d8_count.load() != before ? 1 : 0;
    PG_CHECK_HIP(hipMemcpy(out, dout, no * nbatch * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(flags_out, dflag, nbatch * sizeof(int), hipMemcpyDeviceToHost));
  });
}

// launches of the leg-8 chained-pair kernel by this process
extern "C" long pepsgpu_diag_chain_d8_launches(void) { return tg_chain_d8_count.load(); }
// the counters of PEPSGPU_CHAIN_D8_STATS=1: out2 = {walkers the leg-8 kernel computed, of them walked in chunks}; zeros when unset
extern "C" int pepsgpu_diag_chain_d8_stats(unsigned long long *out2) {
  return guarded(nullptr, [&]() {
    out2[0] = out2[1] = 0;
    if (const unsigned long long *p = tgemm_chain_d8_stats()) {
      PG_CHECK_HIP(hipDeviceSynchronize());
      PG_CHECK_HIP(hipMemcpy(out2, p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
  });
}

template <typename T>
static void diag_chol_t(const double *G, int n, int nbatch, void *Rout) {
  double *dG;
  T *dR;
  size_t ne = (size_t)n * n * nbatch;
  PG_CHECK_HIP(hipMalloc(&dG, ne * sizeof(double)));
  PG_CHECK_HIP(hipMalloc(&dR, ne * sizeof(T)));
  PG_CHECK_HIP(hipMemcpy(dG, G, ne * sizeof(double), hipMemcpyHostToDevice));
  launch_chol_upper<T>(0, nbatch, dG, (long)n * n, n, dR, (long)n * n, (int *)nullptr);
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(Rout, dR, ne * sizeof(T), hipMemcpyDeviceToHost));
  (void)hipFree(dG); (void)hipFree(dR);
}
// rank-adaptive path of the absorption: chol_lowrank_kernel, then chol_upper_kernel for the flagged walkers
template <typename T>
static void diag_chol_adaptive_t(const double *G, int n, int nbatch, void *Rout, int32_t *mlive) {
  double *dG;
  T *dR;
  int *dml;
  size_t ne = (size_t)n * n * nbatch;
  PG_REQUIRE(n <= 256 * CH_LR_Q, 1, "n too large for the low-rank Cholesky");
  PG_CHECK_HIP(hipMalloc(&dG, ne * sizeof(double)));
  PG_CHECK_HIP(hipMalloc(&dR, ne * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dml, nbatch * sizeof(int)));
  PG_CHECK_HIP(hipMemcpy(dG, G, ne * sizeof(double), hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemset(dR, 0, ne * sizeof(T)));
  const size_t lsm = chol_lowrank_smem_bytes(n), smem = chol_smem_bytes(n);
  allow_dynamic_lds(reinterpret_cast<const void *>(&chol_lowrank_kernel<T>), lsm);
  allow_dynamic_lds(reinterpret_cast<const void *>(&chol_upper_kernel<T>), smem);
  hipLaunchKernelGGL(chol_lowrank_kernel<T>, dim3(nbatch), dim3(256), lsm, 0, (const double *)dG, (long)n * n, n, dR,
                     (long)n * n, dml);
  PG_CHECK_HIP(hipGetLastError());
  launch_chol_upper<T>(0, nbatch, dG, (long)n * n, n, dR, (long)n * n, dml, 1);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(Rout, dR, ne * sizeof(T), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(mlive, dml, nbatch * sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(dG); (void)hipFree(dR); (void)hipFree(dml);
}
extern "C" int pepsgpu_diag_chol_adaptive(int dtype_out, const double *G, int n, int nbatch, void *R_out, int32_t *mlive_out) {
  return guarded(nullptr, [&]() {
    if (dtype_out == 0) diag_chol_adaptive_t<float>(G, n, nbatch, R_out, mlive_out);
    else diag_chol_adaptive_t<double>(G, n, nbatch, R_out, mlive_out);
  });
}
// gram_chol_lowrank_kernel alone: P = [nbatch][K][n] of type T; mlive_out[b] = -1 where it declines
template <typename T, int KCAP>
static void diag_gram_chol_t(const void *P, int K, int n, int nbatch, void *Rout, int32_t *mlive) {
  T *dP, *dR;
  int *dml;
  PG_REQUIRE(n <= 256, 1, "n too large for the fused low-rank kernel");
  PG_CHECK_HIP(hipMalloc(&dP, (size_t)K * n * nbatch * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dR, (size_t)n * n * nbatch * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dml, nbatch * sizeof(int)));
  PG_CHECK_HIP(hipMemcpy(dP, P, (size_t)K * n * nbatch * sizeof(T), hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemset(dR, 0, (size_t)n * n * nbatch * sizeof(T)));
  const int npass = K > KCAP ? 4 : 1;          // the multi-pass use of the absorption when a pass cannot hold all rows
  // per-walker live row count = rows up to the last non-zero one, as the absorption passes it (mixed counts in one launch:
  // the short first pass, the walkers it hands on and the multi-pass path all run)
  std::vector<int> hk(nbatch, 0);
  for (int b = 0; b < nbatch; ++b)
    for (int r = 0; r < K; ++r) {
      const T *row = (const T *)P + ((size_t)b * K + r) * n;
      for (int c = 0; c < n; ++c)
        if (row[c] != T(0)) { hk[b] = r + 1; break; }
    }
  int *dk;
  PG_CHECK_HIP(hipMalloc(&dk, nbatch * sizeof(int)));
  PG_CHECK_HIP(hipMemcpy(dk, hk.data(), nbatch * sizeof(int), hipMemcpyHostToDevice));
  launch_gram_chol_lowrank<T, KCAP>(0, nbatch, (const T *)dP, (long)K * n, n, (const int *)dk, 1, K, dR, (long)n * n, dml, 1,
                                    (const int *)nullptr, npass);
  PG_CHECK_HIP(hipDeviceSynchronize());
  (void)hipFree(dk);
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(Rout, dR, (size_t)n * n * nbatch * sizeof(T), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(mlive, dml, nbatch * sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(dP); (void)hipFree(dR); (void)hipFree(dml);
}
extern "C" int pepsgpu_diag_gram_chol(int dtype, const void *P, int K, int n, int nbatch, void *R_out, int32_t *mlive_out) {
  return guarded(nullptr, [&]() {
    if (dtype == 0) diag_gram_chol_t<float, 96>(P, K, n, nbatch, R_out, mlive_out);
    else diag_gram_chol_t<double, 48>(P, K, n, nbatch, R_out, mlive_out);
  });
}
// One of the two one-wave factor kernels alone (form 0: gram_chol_wave_kernel, 1: gram_chol_wave_split_kernel), then the list
// kernel for the walkers it hands on: P = [nbatch][K][n] f32, klive[b] live rows, columns (outer, inner) with inner_live[b]
// (optional) live inner indices; mlive_out[b] < 0 where the list kernel declines as well
extern "C" int pepsgpu_diag_gram_chol_wave(const float *P, int K, int n, int nbatch, const int32_t *klive, int inner,
                                           const int32_t *inner_live, int max_pass, int form, float *R_out, int32_t *mlive_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(K >= 1 && n >= 1 && n <= 256 && nbatch >= 1 && inner >= 1 && n % inner == 0 && max_pass >= 1 && klive, 1, "bad sizes");
    PG_REQUIRE(form == 0 || form == 1, 1, "form is 0 or 1");
    const size_t np = (size_t)K * n * nbatch, nr = (size_t)n * n * nbatch;
    float *dP, *dR;
    int *dml, *dk, *dil = nullptr, *dl;
    PG_CHECK_HIP(hipMalloc(&dP, np * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dR, nr * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dml, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dk, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dl, (nbatch + 1) * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dP, P, np * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dR, R_out, nr * sizeof(float), hipMemcpyHostToDevice));     // what no kernel stores comes back as it went in
    PG_CHECK_HIP(hipMemcpy(dk, klive, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dml, 0xff, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemset(dl, 0, (nbatch + 1) * sizeof(int)));
    if (inner_live) {
      PG_CHECK_HIP(hipMalloc(&dil, nbatch * sizeof(int)));
      PG_CHECK_HIP(hipMemcpy(dil, inner_live, nbatch * sizeof(int), hipMemcpyHostToDevice));
    }
    launch_gram_chol_wave(0, form != 0, nbatch, (const float *)dP, (long)K * n, n, (const int *)dk, 1, K, dR, (long)n * n, dml, inner,
                          (const int *)dil, max_pass, dl);
    PG_CHECK_HIP(hipGetLastError());
    if (n <= 128)
      hipLaunchKernelGGL((gram_chol_lowrank_list_kernel<float, 96, 128>), dim3(std::min(nbatch, 512)), dim3(128), 0, 0, (const float *)dP,
                         (long)K * n, n, (const int *)dk, 1, K, dR, (long)n * n, dml, inner, (const int *)dil, 2, max_pass, (const int *)dl,
                         (const int *)(dl + nbatch));
    else
      hipLaunchKernelGGL((gram_chol_lowrank_list_kernel<float, 96, 256>), dim3(std::min(nbatch, 512)), dim3(256), 0, 0, (const float *)dP,
                         (long)K * n, n, (const int *)dk, 1, K, dR, (long)n * n, dml, inner, (const int *)dil, 2, max_pass, (const int *)dl,
                         (const int *)(dl + nbatch));
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(R_out, dR, nr * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(mlive_out, dml, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dP); (void)hipFree(dR); (void)hipFree(dml); (void)hipFree(dk); (void)hipFree(dl); if (dil) (void)hipFree(dil);
  });
}
// gram_cols_f64_kernel alone: P = [nbatch][K][n] of type T, klive[b] (optional) = live rows; G_out = [nbatch][n][n] float64,
// blocks on or above the diagonal (64 x 64 granularity) written, the rest left at zero
template <typename T>
static void diag_gram_cols_t(const void *P, int K, int n, int nbatch, const int32_t *klive, double *G) {
  T *dP;
  double *dG;
  int *dk = nullptr;
  PG_CHECK_HIP(hipMalloc(&dP, (size_t)K * n * nbatch * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dG, (size_t)n * n * nbatch * sizeof(double)));
  PG_CHECK_HIP(hipMemcpy(dP, P, (size_t)K * n * nbatch * sizeof(T), hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemset(dG, 0, (size_t)n * n * nbatch * sizeof(double)));
  if (klive) {
    PG_CHECK_HIP(hipMalloc(&dk, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dk, klive, nbatch * sizeof(int), hipMemcpyHostToDevice));
  }
  launch_gram_cols_f64<T>(0, nbatch, (const T *)dP, (long)K * n, n, n, (const int *)dk, 1, K, dG, (const int *)nullptr, 1,
                          (const int *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr);
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(G, dG, (size_t)n * n * nbatch * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(dP); (void)hipFree(dG); if (dk) (void)hipFree(dk);
}
extern "C" int pepsgpu_diag_gram_cols(int dtype, const void *P, int K, int n, int nbatch, const int32_t *klive, double *G_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(K >= 1 && n >= 1 && n <= 256 && nbatch >= 1, 1, "bad sizes");
    if (dtype == 0) diag_gram_cols_t<float>(P, K, n, nbatch, klive, G_out); else diag_gram_cols_t<double>(P, K, n, nbatch, klive, G_out);
  });
}
// gram_rows_f64_kernel alone: G[b] = M[b] M[b]^T for the first nrows[b] rows of M (n x K f32, K % 16 == 0), upper 64 x 64 blocks
extern "C" int pepsgpu_diag_gram_rows(const float *M, int n, int K, int nbatch, const int32_t *nrows, double *G_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(n >= 1 && n <= 256 && K >= 16 && K % 16 == 0 && nbatch >= 1 && nrows, 1, "bad sizes");
    float *dM; double *dG; int *dn;
    const size_t ne = (size_t)n * K * nbatch;
    PG_CHECK_HIP(hipMalloc(&dM, ne * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dG, (size_t)n * n * nbatch * sizeof(double)));
    PG_CHECK_HIP(hipMalloc(&dn, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dM, M, ne * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dn, nrows, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dG, 0, (size_t)n * n * nbatch * sizeof(double)));
    launch_gram_rows_f64<float>(0, nbatch, dM, (long)n * K, K, n, dn, dG, (long)n * n, n, nullptr, nullptr, nullptr);
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(G_out, dG, (size_t)n * n * nbatch * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(dM); (void)hipFree(dG); (void)hipFree(dn);
  });
}
// mgemm_dense_kernel alone: M[b] = R[b] Tt[b] with per-walker live rows / a / k2 (nullable), Tt stored [la][u][k2] or [la][k2][u]
extern "C" int pepsgpu_diag_mgemm_dense(const float *R, const float *Tt, int m, int la, int a_dim, int u_dim, int k2_dim, int tt_u_inner,
                                        int nbatch, const int32_t *m_live, const int32_t *a_live, const int32_t *k2_live, float *M_out) {
  return guarded(nullptr, [&]() {
    const int uk = u_dim * k2_dim;
    float *dR, *dT, *dM;
    int *dl[3] = {nullptr, nullptr, nullptr};
    const int32_t *hl[3] = {m_live, a_live, k2_live};
    PG_CHECK_HIP(hipMalloc(&dR, (size_t)m * la * nbatch * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dT, (size_t)la * uk * nbatch * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dM, (size_t)m * uk * nbatch * sizeof(float)));
    PG_REQUIRE(mgemm_dense_ok(m, la, a_dim, u_dim, k2_dim, (long)m * la, (long)la * uk, dR, dT), 1, "shape not supported by mgemm_dense_kernel");
    PG_CHECK_HIP(hipMemcpy(dR, R, (size_t)m * la * nbatch * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dT, Tt, (size_t)la * uk * nbatch * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dM, 0xFF, (size_t)m * uk * nbatch * sizeof(float)));      // NaN pattern: rows beyond the live count stay untouched
    for (int q = 0; q < 3; ++q)
      if (hl[q]) {
        PG_CHECK_HIP(hipMalloc(&dl[q], nbatch * sizeof(int)));
        PG_CHECK_HIP(hipMemcpy(dl[q], hl[q], nbatch * sizeof(int), hipMemcpyHostToDevice));
      }
    launch_mgemm_dense(0, nbatch, dR, (long)m * la, dT, (long)la * uk, dM, (long)m * uk, m, la, a_dim, u_dim, k2_dim, tt_u_inner, dl[0], 1, dl[1],
                       dl[2], nullptr, nullptr, getenv("PEPSGPU_DIAG_TRI") && atoi(getenv("PEPSGPU_DIAG_TRI")) ? 1 : 0);
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(M_out, dM, (size_t)m * uk * nbatch * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(dR); (void)hipFree(dT); (void)hipFree(dM);
    for (int q = 0; q < 3; ++q) if (dl[q]) (void)hipFree(dl[q]);
  });
}
// PEPSGPU_CG_STATS=1: read and reset the per-phase counters of colgram_dense_kernel (trunc_mid.h: cg_stats_dev), launches of >= 1024 walkers
extern "C" int pepsgpu_diag_cg_stats(double *out16) {
  return guarded(nullptr, [&]() {
    unsigned long long h[16] = {0};
    unsigned long long *d = cg_stats_dev();
    if (d) {
      PG_CHECK_HIP(hipDeviceSynchronize());
      PG_CHECK_HIP(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
      PG_CHECK_HIP(hipMemset(d, 0, sizeof(h)));
    }
    for (int i = 0; i < 16; ++i) out16[i] = (double)h[i];
  });
}
// The two LDS-resident Gram + Cholesky kernels alone (trunc_mid.h), f32:
//   which = 0: mid_gram_chol_kernel    X = [nbatch][n][K]  (rows of M),   R^T R = X X^T  (n x n),  nlive[b] = live rows of X
//   which = 1: colgram_dense_kernel    X = [nbatch][K][n]  (rows of P),   R^T R = X^T X  (n x n),  nlive[b] = live rows of X (<= K)
// R_out = [nbatch][n][n] (rows beyond mlive_out[b] untouched = NaN pattern), mlive_out[b] = rows of the factor.
extern "C" int pepsgpu_diag_lds_gram_chol(int which, const float *X, int n, int K, int nbatch, const int32_t *nlive, float *R_out,
                                          int32_t *mlive_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE((which == 0 || which == 1) && n >= 1 && n <= 128 && K >= 1 && nbatch >= 1 && nlive, 1, "bad sizes");
    float *dX, *dR; int *dn, *dm;
    const size_t ne = (size_t)n * K * nbatch, nr = (size_t)n * n * nbatch;
    PG_CHECK_HIP(hipMalloc(&dX, ne * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dR, nr * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dn, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dm, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dX, X, ne * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dn, nlive, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dR, 0xFF, nr * sizeof(float)));
    PG_CHECK_HIP(hipMemset(dm, 0xFF, nbatch * sizeof(int)));
    if (which == 0)
      launch_mid_gram_chol<float>(0, nbatch, dX, (long)n * K, K, dn, nullptr, n, dR, (long)n * n, dm);
    else
      launch_colgram_chol<float>(0, nbatch, dX, (long)n * K, n, dn, 1, K, dR, (long)n * n, dm, 1, nullptr, -4, true);
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(R_out, dR, nr * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(mlive_out, dm, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dX); (void)hipFree(dR); (void)hipFree(dn); (void)hipFree(dm);
  });
}
// The first compression of the dense truncation route as it runs (round 6): G = X X^T on the i8 matrix cores with both triangles written
// (gram_i8.h, sym) + the diagonally pivoted factorisation stopped after kcap rows (chol_pivot.h).  X = [nbatch][n][K] f32 (rows of M),
// 128 < n <= 256, K a multiple of 16; nlive[b] = live rows.  R_out = [nbatch][kcap][n] (rows in pivot order; rows beyond mlive_out[b]
// untouched = NaN pattern).
extern "C" int pepsgpu_diag_chol_pivot(const float *X, int n, int K, int nbatch, const int32_t *nlive, int kcap, float *R_out,
                                       int32_t *mlive_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(n > 128 && n <= 256 && K >= 16 && K % 16 == 0 && nbatch >= 1 && nlive && kcap >= 1 && kcap <= 64, 1, "bad sizes");
    float *dX, *dR; int *dn, *dm; double *dG;
    const size_t ne = (size_t)n * K * nbatch, nr = (size_t)64 * n * nbatch;
    PG_CHECK_HIP(hipMalloc(&dX, ne * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dR, nr * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dG, (size_t)n * n * nbatch * sizeof(double)));
    PG_CHECK_HIP(hipMalloc(&dn, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dm, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dX, X, ne * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dn, nlive, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dR, 0xFF, nr * sizeof(float)));
    PG_CHECK_HIP(hipMemset(dG, 0xFF, (size_t)n * n * nbatch * sizeof(double)));
    PG_CHECK_HIP(hipMemset(dm, 0xFF, nbatch * sizeof(int)));
    PG_REQUIRE(gram_rows_i8_ok(dX, n), 1, "the i8 row Gram does not take this shape");
    launch_gram_rows_f64<float>(0, nbatch, dX, (long)n * K, K, n, dn, dG, (long)n * n, n, nullptr, nullptr, nullptr, 1);
    launch_chol_pivot<float>(0, nbatch, dG, (long)n * n, n, dR, (long)64 * n, dm, n, dn, 1, nullptr, kcap);
    PG_CHECK_HIP(hipDeviceSynchronize());
    std::vector<float> h(nr);
    PG_CHECK_HIP(hipMemcpy(h.data(), dR, nr * sizeof(float), hipMemcpyDeviceToHost));
    for (int b = 0; b < nbatch; ++b)
      memcpy(R_out + (size_t)b * kcap * n, h.data() + (size_t)b * 64 * n, sizeof(float) * (size_t)kcap * n);
    PG_CHECK_HIP(hipMemcpy(mlive_out, dm, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dX); (void)hipFree(dR); (void)hipFree(dG); (void)hipFree(dn); (void)hipFree(dm);
  });
}
// rows_qr_kernel alone (round 6): X = [nbatch][k][len] f32 nearly orthogonal rows by decreasing norm, klive[b] = rows that exist;
// V_out = [nbatch][k][len] orthonormal rows spanning the same space (live rows first, the rest zero), klive_out[b] = their count.
extern "C" int pepsgpu_diag_rows_qr(const float *X, int k, int len, int nbatch, const int32_t *klive, float *V_out, int32_t *klive_out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(rows_qr_ok(k, len) && nbatch >= 1 && klive, 1, "bad sizes");
    float *dX, *dV; int *dn, *dm;
    const size_t ne = (size_t)k * len * nbatch;
    PG_CHECK_HIP(hipMalloc(&dX, ne * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dV, ne * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dn, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dm, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dX, X, ne * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dn, klive, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemset(dV, 0xFF, ne * sizeof(float)));
    PG_CHECK_HIP(hipMemset(dm, 0xFF, nbatch * sizeof(int)));
    launch_rows_qr(0, nbatch, dX, (long)k * len, k, len, dn, dV, (long)k * len, dm, nullptr);
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(V_out, dV, ne * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(klive_out, dm, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dX); (void)hipFree(dV); (void)hipFree(dn); (void)hipFree(dm);
  });
}
// trace_dot4_kernel alone: out[b] = exp(lsum[b]) sum_{ijkl} a[b][i][j][k][l] b[b][l][k][j][i], 0.0 where flag[b] >= 0
template <typename T>
static void diag_dot4_t(const void *a, const void *b, const int *dims4, int nbatch, const double *lsum, const int32_t *flag, double *out) {
  typedef typename acc64_of<T>::type Acc;
  constexpr int ko = (int)(sizeof(Acc) / sizeof(double));
  const long n = (long)dims4[0] * dims4[1] * dims4[2] * dims4[3];
  const size_t bytes = sizeof(T) * (size_t)n * nbatch;
  T *da, *db; double *dl, *dout; int *df = nullptr;
  PG_CHECK_HIP(hipMalloc(&da, bytes));
  PG_CHECK_HIP(hipMalloc(&db, bytes));
  PG_CHECK_HIP(hipMalloc(&dl, nbatch * sizeof(double)));
  PG_CHECK_HIP(hipMalloc(&dout, (size_t)ko * nbatch * sizeof(double)));
  PG_CHECK_HIP(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
  PG_CHECK_HIP(hipMemcpy(dl, lsum, nbatch * sizeof(double), hipMemcpyHostToDevice));
  if (flag) {
    PG_CHECK_HIP(hipMalloc(&df, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(df, flag, nbatch * sizeof(int), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL((trace_dot4_kernel<T, Acc>), dim3(nbatch), dim3(256), 0, 0, (const T *)da, (const T *)db, n, dims4[0], dims4[1],
                     dims4[2], dims4[3], (const double *)dl, (const int *)df, 1, 0, 0, 1L, dout);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(out, dout, (size_t)ko * nbatch * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dl); (void)hipFree(dout); if (df) (void)hipFree(df);
}
extern "C" int pepsgpu_diag_dot4(int dtype, const void *a, const void *b, const int *dims4, int nbatch, const double *lsum,
                                 const int32_t *flag, double *out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(a && b && dims4 && lsum && out && nbatch >= 1, 1, "bad arguments");
    PG_REQUIRE(dims4[0] >= 1 && dims4[1] >= 1 && dims4[2] >= 1 && dims4[3] >= 1 &&
                   (double)dims4[0] * dims4[1] * dims4[2] * dims4[3] * nbatch < 2147483648.0, 1, "bad sizes");
    if (dtype == PEPSGPU_F32) diag_dot4_t<float>(a, b, dims4, nbatch, lsum, flag, out);
    else if (dtype == PEPSGPU_F64) diag_dot4_t<double>(a, b, dims4, nbatch, lsum, flag, out);
    else if (dtype == PEPSGPU_C128) diag_dot4_t<c128>(a, b, dims4, nbatch, lsum, flag, out);
    else throw Error(1, "unknown dtype");
  });
}
// The device's SuwaTodoStateUpdate alone (round 6): a chain of `steps` updates on one weight vector (n <= 16 states), fed with the
// raw 32-bit outputs of the caller's std::mt19937 (two per step, the reference's long double draw); out_chain[s] = the state after step s.
extern "C" int pepsgpu_diag_suwa_todo(const double *weights, int n, int init, const uint32_t *words, int steps, int32_t *out_chain) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(weights && words && out_chain && n >= 1 && n <= SW_MAXC && init >= 0 && init < n && steps >= 1, 1, "bad arguments");
    double *dw; unsigned *dd; int *dout;
    PG_CHECK_HIP(hipMalloc(&dw, n * sizeof(double)));
    PG_CHECK_HIP(hipMalloc(&dd, 2 * (size_t)steps * sizeof(unsigned)));
    PG_CHECK_HIP(hipMalloc(&dout, (size_t)steps * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dw, weights, n * sizeof(double), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dd, words, 2 * (size_t)steps * sizeof(unsigned), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sweep_suwa_todo_chain_kernel, dim3(1), dim3(64), 0, 0, (const double *)dw, n, init, (const unsigned *)dd, steps, dout);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(out_chain, dout, (size_t)steps * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dw); (void)hipFree(dd); (void)hipFree(dout);
  });
}
extern "C" int pepsgpu_diag_chol(int dtype_out, const double *G, int n, int nbatch, void *R_out) {
  return guarded(nullptr, [&]() {
    if (dtype_out == 0) diag_chol_t<float>(G, n, nbatch, R_out); else diag_chol_t<double>(G, n, nbatch, R_out);
  });
}

template <typename T>
static void diag_jacobi_t(void *M, int m, int len, int nbatch, int k, void *Vt, void *S, int force_global, int *sweeps) {
  T *dM, *dV, *dS;
  int *dsw;
  size_t ne = (size_t)m * len * nbatch;
  PG_CHECK_HIP(hipMalloc(&dM, ne * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dV, (size_t)k * len * nbatch * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dS, (size_t)k * nbatch * sizeof(T)));
  PG_CHECK_HIP(hipMalloc(&dsw, nbatch * sizeof(int)));
  PG_CHECK_HIP(hipMemcpy(dM, M, ne * sizeof(T), hipMemcpyHostToDevice));
  const size_t need = sizeof(T) * (size_t)m * (len | 1);
  const int use_lds = !force_global && need <= JACOBI_LDS_MAX;
  if (use_lds) allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), need);
  if (sizeof(T) == 4 && force_global == 2) {
    PG_REQUIRE(m <= 256 && len <= 256, 1, "register Jacobi handles up to 256 x 256");
    hipLaunchKernelGGL(jacobi_rows_reg256_kernel, dim3(nbatch), dim3(512), 0, 0, (float *)dM, (long)m * len, m, len, len,
                       40, dsw, (const int *)nullptr, 1, 0);
  } else if (sizeof(T) == 4 && force_global >= 5 && force_global <= 8) {
    // 16-lanes-per-row tournament: 5 = four waves (128 rows), 6 = two (64), rows up to 128 long; 7 / 8 = the same with rows up to 256 long
    const int wide = force_global >= 7, four = force_global == 5 || force_global == 7;
    PG_REQUIRE(m <= (four ? 128 : 64) && len <= (wide ? 256 : 128), 1, "grouped tournament handles up to 128 (64) x 128 (256)");
    if (force_global == 5) launch_jacobi_grp<4, 8>(0, nbatch, (float *)dM, (long)m * len, m, len, len, 40, dsw, (const int *)nullptr, 1, 0);
    else if (force_global == 6) launch_jacobi_grp<2, 8>(0, nbatch, (float *)dM, (long)m * len, m, len, len, 40, dsw, (const int *)nullptr, 1, 0);
    else if (force_global == 7) launch_jacobi_grp<4, 16>(0, nbatch, (float *)dM, (long)m * len, m, len, len, 40, dsw, (const int *)nullptr, 1, 0);
    else launch_jacobi_grp<2, 16>(0, nbatch, (float *)dM, (long)m * len, m, len, len, 40, dsw, (const int *)nullptr, 1, 0);
  } else if (sizeof(T) == 4 && (force_global == 9 || force_global == 10)) {
    // the same tournament with ONE wave per walker (up to 32 rows): 9 = rows up to 128 long, 10 = up to 256 (polish of 17..32 rows,
    // every walker of a small batch)
    PG_REQUIRE(m <= 32 && len <= (force_global == 9 ? 128 : 256), 1, "one-wave grouped tournament handles up to 32 x 128 (256)");
    if (force_global == 9) launch_jacobi_grp<1, 8>(0, nbatch, (float *)dM, (long)m * len, m, len, len, 40, dsw, (const int *)nullptr, 1, 0);
    else launch_jacobi_grp<1, 16>(0, nbatch, (float *)dM, (long)m * len, m, len, len, 40, dsw, (const int *)nullptr, 1, 0);
  } else if (sizeof(T) == 4 && force_global == 3) {   // one-wave-per-walker kernel (up to 32 x 256)
    PG_REQUIRE(m <= JR_SMALL_ROWS && len <= 256, 1, "small Jacobi handles up to 32 x 256");
    // per-walker live row count = rows up to the last non-zero one (mixed counts inside a launch, as in the absorption)
    std::vector<int> hm(nbatch, 0);
    for (int b = 0; b < nbatch; ++b)
      for (int r = 0; r < m; ++r) {
        const T *row = (const T *)M + ((size_t)b * m + r) * len;
        for (int c = 0; c < len; ++c)
          if (row[c] != T(0)) { hm[b] = r + 1; break; }
      }
    int *dm;
    PG_CHECK_HIP(hipMalloc(&dm, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dm, hm.data(), nbatch * sizeof(int), hipMemcpyHostToDevice));
    if (m <= JR_BR && len <= 64)      // as the absorption: short rows -> four walkers per wave, 16 lanes x 4 columns
      hipLaunchKernelGGL((jacobi_rows_tiny4_kernel<4>), dim3((nbatch + 15) / 16), dim3(256), 0, 0, (float *)dM, (long)m * len, m, len,
                         len, 40, dsw, (const int *)dm, 1, nbatch, JrSelect());
    else if (m <= JR_BR && len <= 128)   // ... 16 lanes x 8 columns
      hipLaunchKernelGGL((jacobi_rows_tiny4_kernel<8>), dim3((nbatch + 15) / 16), dim3(256), 0, 0, (float *)dM, (long)m * len, m, len,
                         len, 40, dsw, (const int *)dm, 1, nbatch, JrSelect());
    else if (m <= JR_BR)     // <= 16 rows -> tiny kernel, 17..32 -> small kernel
      hipLaunchKernelGGL(jacobi_rows_tiny_kernel, dim3((nbatch + 3) / 4), dim3(256), 0, 0, (float *)dM, (long)m * len, m, len,
                         len, 40, dsw, (const int *)dm, 1, nbatch);
    else
      hipLaunchKernelGGL(jacobi_rows_small_kernel, dim3((nbatch + 3) / 4), dim3(256), 0, 0, (float *)dM, (long)m * len, m, len,
                         len, 40, dsw, (const int *)dm, 1, nbatch, 0);
    PG_CHECK_HIP(hipDeviceSynchronize());
    (void)hipFree(dm);
  } else {
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nbatch), dim3(1024), use_lds ? need : 0, 0, dM, (long)m * len, m, len,
                       len, 40, use_lds, dsw, (const int *)nullptr, 1);
  }
  PG_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nbatch), dim3(256), 0, 0, (const T *)dM, (long)m * len, m, len, len, k,
                     dV, (long)k * len, dS, (long)k, (const int *)nullptr, 1);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipDeviceSynchronize());
  PG_CHECK_HIP(hipMemcpy(M, dM, ne * sizeof(T), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(Vt, dV, (size_t)k * len * nbatch * sizeof(T), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(S, dS, (size_t)k * nbatch * sizeof(T), hipMemcpyDeviceToHost));
  if (sweeps) PG_CHECK_HIP(hipMemcpy(sweeps, dsw, nbatch * sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(dM); (void)hipFree(dV); (void)hipFree(dS); (void)hipFree(dsw);
}
// complex float64: the general complex Jacobi as absorb_simple launches it (60 sweeps at most), then the select; S comes back real
static void diag_jacobi_cplx(void *M, int m, int len, int nbatch, int k, void *Vt, void *S, int *sweeps) {
  DevBufs bufs;
  const size_t ne = (size_t)m * len * nbatch, nv = (size_t)k * len * nbatch, ns = (size_t)k * nbatch;
  c128 *dM = bufs.alloc<c128>(ne, M), *dV = bufs.alloc<c128>(nv), *dS = bufs.alloc<c128>(ns);
  int *dsw = bufs.alloc<int>(nbatch);
  hipLaunchKernelGGL(jacobi_rows_cplx_kernel<c128>, dim3(nbatch), dim3(1024), 0, 0, dM, (long)m * len, m, len, len, 60, dsw,
                     (const int *)nullptr, 1);
  PG_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(select_rows_kernel<c128>, dim3(nbatch), dim3(256), 0, 0, (const c128 *)dM, (long)m * len, m, len, len, k, dV,
                     (long)k * len, dS, (long)k, (const int *)nullptr, 1);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipDeviceSynchronize());
  std::vector<c128> hs(ns);
  PG_CHECK_HIP(hipMemcpy(M, dM, ne * sizeof(c128), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(Vt, dV, nv * sizeof(c128), hipMemcpyDeviceToHost));
  PG_CHECK_HIP(hipMemcpy(hs.data(), dS, ns * sizeof(c128), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < ns; ++e) ((double *)S)[e] = hs[e].re;
  if (sweeps) PG_CHECK_HIP(hipMemcpy(sweeps, dsw, nbatch * sizeof(int), hipMemcpyDeviceToHost));
}
extern "C" int pepsgpu_diag_jacobi(int dtype, void *M, int m, int len, int nbatch, int k, void *Vt, void *S, int force_global,
                        int *sweeps) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(m >= 1 && len >= 1 && nbatch >= 1 && k >= 1 && m <= 1024 && k <= m, 1, "bad sizes");
    if (dtype == 0) diag_jacobi_t<float>(M, m, len, nbatch, k, Vt, S, force_global, sweeps);
    else if (dtype == 1) diag_jacobi_t<double>(M, m, len, nbatch, k, Vt, S, force_global, sweeps);
    else if (dtype == PEPSGPU_C128) diag_jacobi_cplx(M, m, len, nbatch, k, Vt, S, sweeps);
    else throw Error(1, "unknown dtype");
  });
}

// ---- the pieces only the float64 / complex dense truncation routes launch (rows_qr.h), one launch each ----
// One Cholesky-QR pass X <- L^-1 X, L L^H = S: S = [nbatch][64][64] (upper triangle read), X = [nbatch][r_max][len] in place.
// float64: rows[b] rows per entry (chol_solve_rows_kernel); complex: r rows for every entry (chol_solve_rows_cplx_kernel).
extern "C" int pepsgpu_diag_chol_solve_rows(int is_complex, const void *S, void *X, int nbatch, int r_max, int len, const int32_t *rows,
                                            int r, const int32_t *run_flag) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(S && X && nbatch >= 1 && r_max >= 1 && r_max <= CS_K && len >= 1, 1, "diag_chol_solve_rows: bad sizes (r_max <= 64)");
    if (is_complex) PG_REQUIRE(r >= 0 && r <= r_max, 1, "diag_chol_solve_rows: r must be in [0, r_max]");
    else {
      PG_REQUIRE(rows != nullptr, 1, "diag_chol_solve_rows: rows is null");
      for (int b = 0; b < nbatch; ++b) PG_REQUIRE(rows[b] >= 0 && rows[b] <= r_max, 1, "diag_chol_solve_rows: rows[b] must be in [0, r_max]");
    }
    DevBufs bufs;
    const size_t es = is_complex ? sizeof(c128) : sizeof(double);
    const size_t nS = (size_t)nbatch * CS_K * CS_K, nX = (size_t)nbatch * r_max * len;
    char *dS = bufs.alloc<char>(nS * es, S), *dX = bufs.alloc<char>(nX * es, X);
    int *dflag = run_flag ? bufs.alloc<int>(nbatch, run_flag) : nullptr;
    if (is_complex) {
      hipLaunchKernelGGL(chol_solve_rows_cplx_kernel, dim3(nbatch), dim3(256), 0, 0, (const c128 *)dS, (long)CS_K * CS_K, CS_K, (c128 *)dX,
                         (long)r_max * len, len, r, (const int *)dflag);
    } else {
      int *drows = bufs.alloc<int>(nbatch, rows);
      hipLaunchKernelGGL(chol_solve_rows_kernel, dim3(nbatch), dim3(256), 0, 0, (const double *)dS, (long)CS_K * CS_K, CS_K, (double *)dX,
                         (long)r_max * len, len, (const int *)drows, (const int *)dflag);
    }
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(X, dX, nX * es, hipMemcpyDeviceToHost));
  });
}
// gather_rows_kernel as the pivoted route launches it (64 slots per entry): Q[b][j] = M[b][piv[b][j]] for j < rows[b], piv >= 0;
// M = [nbatch][m][len], piv = [nbatch][slots], Q = [nbatch][64][len] (read as well: what the kernel leaves comes back unchanged)
extern "C" int pepsgpu_diag_gather_rows(int is_complex, const void *M, int nbatch, int m, int len, const int32_t *piv, int slots,
                                        const int32_t *rows, const int32_t *run_flag, void *Q) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(M && piv && rows && Q && nbatch >= 1 && nbatch <= 65535 && m >= 1 && len >= 1 && slots >= 1, 1, "diag_gather_rows: bad sizes");
    for (int b = 0; b < nbatch; ++b) {
      PG_REQUIRE(rows[b] >= 0 && rows[b] <= std::min(slots, 64), 1, "diag_gather_rows: rows[b] must be in [0, min(slots, 64)]");
      for (int j = 0; j < slots; ++j) PG_REQUIRE(piv[(size_t)b * slots + j] < m, 1, "diag_gather_rows: pivot beyond the rows of M");
    }
    DevBufs bufs;
    const size_t es = is_complex ? sizeof(c128) : sizeof(double);
    const size_t nM = (size_t)nbatch * m * len, nQ = (size_t)nbatch * 64 * len;
    char *dM = bufs.alloc<char>(nM * es, M), *dQ = bufs.alloc<char>(nQ * es, Q);
    int *dpiv = bufs.alloc<int>((size_t)nbatch * slots, piv), *drows = bufs.alloc<int>(nbatch, rows);
    int *dflag = run_flag ? bufs.alloc<int>(nbatch, run_flag) : nullptr;
    if (is_complex)
      hipLaunchKernelGGL(gather_rows_kernel<c128>, dim3(64, nbatch), dim3(256), 0, 0, (const c128 *)dM, (long)m * len, len, (const int *)dpiv,
                         slots, (const int *)drows, (c128 *)dQ, 64L * len, (const int *)dflag);
    else
      hipLaunchKernelGGL(gather_rows_kernel<double>, dim3(64, nbatch), dim3(256), 0, 0, (const double *)dM, (long)m * len, len,
                         (const int *)dpiv, slots, (const int *)drows, (double *)dQ, 64L * len, (const int *)dflag);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(Q, dQ, nQ * es, hipMemcpyDeviceToHost));
  });
}
// sign_table_kernel: out = [rows][cols] of +1 / -1 in the element type
extern "C" int pepsgpu_diag_sign_table(int is_complex, int rows, int cols, void *out) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(out && rows >= 1 && cols >= 1 && (long)rows * cols <= (1L << 24), 1, "diag_sign_table: bad sizes");
    DevBufs bufs;
    const size_t es = is_complex ? sizeof(c128) : sizeof(double), n = (size_t)rows * cols;
    char *d = bufs.alloc<char>(n * es);
    if (is_complex) hipLaunchKernelGGL(sign_table_kernel<c128>, dim3((n + 255) / 256), dim3(256), 0, 0, (c128 *)d, rows, cols);
    else hipLaunchKernelGGL(sign_table_kernel<double>, dim3((n + 255) / 256), dim3(256), 0, 0, (double *)d, rows, cols);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(out, d, n * es, hipMemcpyDeviceToHost));
  });
}
// the truncation of one interior site of a float64 / complex context on given matrices (Engine::diag_truncate_site)
extern "C" int pepsgpu_diag_truncate_site(pepsgpu_ctx *ctx, const void *M, int nbatch, int m, int u, int k2, const int32_t *rows, int route,
                                          void *V_out, int32_t *klive_out, int32_t *route_flag_out) {
  CTX_CALL(ctx->eng->diag_truncate_site(M, nbatch, m, u, k2, rows, route, V_out, klive_out, route_flag_out));
}

// The sel form of the short-row Jacobi alone, as trunc_jacobi launches it on a low-rank site (len <= 64: CPL = 4, else 8).
extern "C" int pepsgpu_diag_trunc_rows(const float *M, int m, int len, int nbatch, const int32_t *rows, int k, int span, float *Vt,
                                       int32_t *klive, int32_t *sweeps) {
  return guarded(nullptr, [&]() {
    PG_REQUIRE(m >= 1 && len >= 1 && len <= 128 && nbatch >= 1 && k >= 1, 1, "bad sizes");
    float *dM, *dV;
    int *dm, *dk, *dsw;
    const size_t ne = (size_t)m * len * nbatch, nv = (size_t)k * len * nbatch;
    PG_CHECK_HIP(hipMalloc(&dM, ne * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dV, nv * sizeof(float)));
    PG_CHECK_HIP(hipMalloc(&dm, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dk, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMalloc(&dsw, nbatch * sizeof(int)));
    PG_CHECK_HIP(hipMemcpy(dM, M, ne * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dV, Vt, nv * sizeof(float), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dm, rows, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dk, klive, nbatch * sizeof(int), hipMemcpyHostToDevice));
    PG_CHECK_HIP(hipMemcpy(dsw, sweeps, nbatch * sizeof(int), hipMemcpyHostToDevice));
    JrSelect sel;
    sel.V = dV; sel.wV = (long)k * len; sel.k = k; sel.klive_out = dk; sel.span = span ? 1 : 0;
    if (len <= 64)
      hipLaunchKernelGGL((jacobi_rows_tiny4_kernel<4>), dim3((nbatch + 15) / 16), dim3(256), 0, 0, dM, (long)m * len, m, len, len, 40, dsw,
                         (const int *)dm, 1, nbatch, sel);
    else
      hipLaunchKernelGGL((jacobi_rows_tiny4_kernel<8>), dim3((nbatch + 15) / 16), dim3(256), 0, 0, dM, (long)m * len, m, len, len, 40, dsw,
                         (const int *)dm, 1, nbatch, sel);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipDeviceSynchronize());
    PG_CHECK_HIP(hipMemcpy(Vt, dV, nv * sizeof(float), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(klive, dk, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    PG_CHECK_HIP(hipMemcpy(sweeps, dsw, nbatch * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dM); (void)hipFree(dV); (void)hipFree(dm); (void)hipFree(dk); (void)hipFree(dsw);
  });
}
