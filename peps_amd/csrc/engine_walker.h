// BMPSWalker on the device (bmps_contractor.h:357-646, bmps/impl/bmps_walker.h:13-465, bten_operations.h:60-277).
//
// The reference forks ONE boundary MPS out of a contractor stack; it evolves on its own -- through rows of the network
// (EvolveStep) or through ANY TransferMPO the caller hands over (Evolve) --, is closed against a named boundary of the opposite
// stack (ContractRow) and keeps its own LEFT / RIGHT BTen caches for multi-site traces on one row.  Here a walker object holds
// the fork for every Monte-Carlo walker of the context at once (a deep copy of the top BMPS: tensors [walker][elements], live
// bond counts, log-scales) plus the two BTen caches; every operation is the same batched launch sequence the contractor's own
// stacks use (absorb_* / bten_step / finish_dot), with the MPO named in one of three ways (pepsgpu_walker_set_mpo):
//   * slice `num` of the network under the walkers' current configurations,
//   * slice `num` with a per-walker state for every site along it (an excited row),
//   * explicit site tensors along the slice (one set shared by the walkers, or one per walker): NOT a row of the network.
// The row operations support the UP walker / DOWN opposite pair only, as the reference does (bmps_walker.h:114-118).
#pragma once
#include "engine.h"
#include "engine_sweep.h"

namespace pepsgpu {

// A map of the states of one site handed to a kernel by value: the two calls below need no upload of their own for it
constexpr int WK_MAXDP = 32;
struct WalkerStateMap { int v[WK_MAXDP]; };

// The site patch of an excited row (walker_set_mpo_excited): state s of site `site` of every walker's table becomes map[s]
__global__ void walker_excite_site_kernel(int *__restrict__ tab, int sites, int site, WalkerStateMap map, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  int *p = tab + (long)w * sites + site;
  *p = map.v[*p];
}

// The candidates of one position of walker_trace_slice from the MPO's state table tab [n][sites]: cand[w] = map[s] for the state s of
// `site`, skip[w] != 0 (the convention of bten_step) where the replacement is the identity or the walker is masked out (mask nullable)
__global__ void walker_trace_cand_kernel(const int *__restrict__ tab, int sites, int site, WalkerStateMap map,
                                         const int *__restrict__ mask, int *__restrict__ cand, int *__restrict__ skip, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int s = tab[(long)w * sites + site], r = map.v[s];
  cand[w] = r;
  skip[w] = (r == s || (mask && !mask[w])) ? 1 : 0;
}

// ---- pair moves on a walker's row (the singlet-pair correlation, singlet_pair_correlation_measurement_mixin.h:349-534) ----
// One slot of a pair table over PHYSICAL states (the layout of pepsgpu_nn_pair_slice_fermion: [d * d][2][2], (-1, -1) for none) handed
// to a kernel by value, as WalkerStateMap: v[(a * d + b) * 2 + site] of the slot, d <= WK_MAXD.  No upload of its own.
constexpr int WK_MAXD = WK_MAXDP / 4;
struct WalkerPairMap { signed char v[2 * WK_MAXD * WK_MAXD]; };

// The candidate of the pair (e1, e2) of extended states on two sites adjacent in row-major order, by the rule of pair_cand_kernel
// (engine_sweep.h): before = v1 ^ n(a), e1' = a' + d (before ^ n(a')), e2' = b' + d (before ^ n(a') ^ n(b')).  Returns the sign
// Sigma(S') / Sigma(S) (+1: fermion number kept, -1: changed by +-2), 0 and (e1, e2) themselves for "no candidate".
__device__ __host__ inline int walker_pair_apply(const WalkerPairMap &m, int d, unsigned occ_bits, int e1, int e2, int *c1, int *c2) {
  const int a = e1 % d, b = e2 % d;
  const int pa = m.v[2 * (a * d + b)], pb = m.v[2 * (a * d + b) + 1];
  *c1 = e1; *c2 = e2;
  if (pa < 0) return 0;
  const int oa = (int)((occ_bits >> a) & 1u), ob = (int)((occ_bits >> b) & 1u);
  const int na = (int)((occ_bits >> pa) & 1u), nb = (int)((occ_bits >> pb) & 1u);
  const int before = ((e1 / d) & 1) ^ oa;
  *c1 = pa + d * (before ^ na);
  *c2 = pb + d * (before ^ na ^ nb);
  return (na + nb == oa + ob) ? 1 : -1;
}

// The two-site patch of an excited row (walker_set_mpo_excited_pair): sites `site`, `site + 1` of every walker's table become the
// candidate of the slot; a walker without it keeps its two states
__global__ void walker_excite_pair_kernel(int *__restrict__ tab, int sites, int site, int d, unsigned occ_bits, WalkerPairMap map, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  int *p = tab + (long)w * sites + site;
  int c1, c2;
  if (walker_pair_apply(map, d, occ_bits, p[0], p[1], &c1, &c2) != 0) { p[0] = c1; p[1] = c2; }
}

// The candidates of one position of walker_pair_trace_slice from the MPO's state table tab [n][sites]: for the sites `site`,
// `site + 1` and the slots k = 0, 1 cand [n][2][2] (slot, site), sign [n][2], skip [2][n] != 0 (the convention of bten_step) where
// the walker has no candidate k or is masked out (mask nullable)
__global__ void walker_pair_cand_kernel(const int *__restrict__ tab, int sites, int site, int d, unsigned occ_bits, WalkerPairMap map0,
                                        WalkerPairMap map1, const int *__restrict__ mask, int *__restrict__ cand,
                                        int *__restrict__ skip, int *__restrict__ sign, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int e1 = tab[(long)w * sites + site], e2 = tab[(long)w * sites + site + 1];
  const bool off = mask && !mask[w];
  for (int k = 0; k < 2; ++k) {
    int c1, c2;
    const int sg = walker_pair_apply(k ? map1 : map0, d, occ_bits, e1, e2, &c1, &c2);
    cand[4 * (long)w + 2 * k] = c1;
    cand[4 * (long)w + 2 * k + 1] = c2;
    sign[2 * (long)w + k] = sg;
    skip[(long)k * n + w] = (sg == 0 || off) ? 1 : 0;
  }
}

// out[w][col] = sign[w * sstride] res[w] exp(lsum[w]) into a ZEROED [n][stride] table of AccT scalars (stored as doubles, complex
// interleaved); a skipped walker keeps the zero of its entry
template <typename AccT>
__global__ void walker_pair_store_kernel(const AccT *__restrict__ res, const double *__restrict__ lsum, const int *__restrict__ sign,
                                         int sstride, const int *__restrict__ skip, double *__restrict__ out, int stride, int col, int n) {
  constexpr int ko = (int)(sizeof(AccT) / sizeof(double));
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n || skip[w]) return;
  sw_put(out + ((long)w * stride + col) * ko, sw_scaled(res[w], (double)sign[(long)w * sstride] * exp(lsum[w])));
}

inline std::atomic<long> &walker_pair_slice_calls() {   // completed walker_pair_trace_slice calls (pepsgpu_diag_walker_pair_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

// occ [d] and a pair table checked as require_pair_tables does (status 1); its two slots as kernel arguments m0 / m1
inline unsigned walker_pair_maps(int d, int dp, const int32_t *occ, const int32_t *pair_table, WalkerPairMap *m0, WalkerPairMap *m1) {
  PG_REQUIRE(occ && pair_table, 1, "BMPSWalker: null pair table");
  PG_REQUIRE(d >= 1 && 4 * d == dp && d <= WK_MAXD, 1, "BMPSWalker: the context's physical dimension must be 4 d (extended states), d <= 8");
  const unsigned occ_bits = require_pair_tables(d, occ, pair_table);
  for (int ab = 0; ab < d * d; ++ab)
    for (int q = 0; q < 2; ++q) {
      m0->v[2 * ab + q] = (signed char)pair_table[4 * ab + q];
      m1->v[2 * ab + q] = (signed char)pair_table[4 * ab + 2 + q];
    }
  return occ_bits;
}

inline std::atomic<long> &walker_slice_calls() {   // completed walker_trace_slice calls of the process (pepsgpu_diag_walker_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

template <typename T>
typename Engine<T>::BMPSDev Engine<T>::copy_bmps(const BMPSDev &b) {
  BMPSDev o;
  o.kmax = b.kmax; o.mlmax = b.mlmax; o.depth = b.depth;
  for (const auto &t : b.t) {
    DTen<T> c = t;
    c.p = (T *)arena_.alloc(sizeof(T) * (size_t)t.n * nw_);
    PG_CHECK_HIP(hipMemcpyAsync(c.p, t.p, sizeof(T) * (size_t)t.n * nw_, hipMemcpyDeviceToDevice, stream_));
    o.t.push_back(c);
  }
  for (int *l : b.live) {
    int *c = nullptr;
    if (l) {
      c = (int *)arena_.alloc(sizeof(int) * nw_);
      PG_CHECK_HIP(hipMemcpyAsync(c, l, sizeof(int) * nw_, hipMemcpyDeviceToDevice, stream_));
    }
    o.live.push_back(c);
  }
  o.logscale = (double *)arena_.alloc(sizeof(double) * nw_);
  PG_CHECK_HIP(hipMemcpyAsync(o.logscale, b.logscale, sizeof(double) * nw_, hipMemcpyDeviceToDevice, stream_));
  return o;
}

template <typename T>
typename Engine<T>::WalkerDev &Engine<T>::walker_ref(int id) {
  auto it = walkers_.find(id);
  PG_REQUIRE(it != walkers_.end(), 1, "BMPSWalker: no such walker");
  return it->second;
}

template <typename T>
void Engine<T>::walker_free_bten(WalkerDev &w) {
  for (auto *v : {&w.btl, &w.btr})
    for (auto &b : *v) { arena_.free(b.t.p); if (b.logscale) arena_.free(b.logscale); }
  w.btl.clear(); w.btr.clear();
  w.lcol = 0; w.rcol = 0;
}

template <typename T>
void Engine<T>::walker_free_mpo(WalkerDev &w) {
  if (w.mpo_cfg) arena_.free(w.mpo_cfg);
  if (w.mpo_tens) arena_.free(w.mpo_tens);
  w.mpo_cfg = nullptr; w.mpo_tens = nullptr; w.mpo_nt = 0; w.mpo_num = -1;
  w.mpo_hrow.clear();
}

template <typename T>
void Engine<T>::walkers_clear() {
  for (auto &kv : walkers_) {
    walker_free_bten(kv.second);
    walker_free_mpo(kv.second);
    free_bmps(kv.second.b);
  }
  walkers_.clear();
}

// GetWalker (bmps_walker.h:51-58): a copy of the top of the stack (level < 0), or BMPSWalker(tn, stack[level], pos, level + 1,
// params) as the structure-factor mixin builds its main walker from the vacuum (structure_factor_measurement_mixin.h:121-122)
template <typename T>
int Engine<T>::walker_create(int pos, int level) {
  require_ready();
  PG_REQUIRE(bmps_size(pos) > 0, 3, "GetWalker: cannot create a walker from an empty BMPS stack");
  PG_REQUIRE(level < bmps_size(pos), 1, "BMPSWalker: level outside the stack");
  const int lv = level < 0 ? bmps_size(pos) - 1 : level;
  WalkerDev w;
  w.pos = pos;
  w.stack = lv + 1;
  w.b = copy_bmps(bmps_[pos][lv]);
  const int id = next_walker_id_++;
  walkers_.emplace(id, std::move(w));
  return id;
}

// copy construction of a walker (`auto excited_walker = main_walker;`): the BMPS and the counters.  The MPO named by walker_set_mpo is
// NOT copied (the reference's walker holds no MPO: Evolve takes it as an argument) -- the copy starts on the network's own slices --
// and its BTen caches start empty
template <typename T>
int Engine<T>::walker_clone(int id) {
  require_ready();
  WalkerDev &src = walker_ref(id);
  WalkerDev w;
  w.pos = src.pos;
  w.stack = src.stack;
  w.b = copy_bmps(src.b);
  const int nid = next_walker_id_++;
  walkers_.emplace(nid, std::move(w));
  return nid;
}

template <typename T>
void Engine<T>::walker_destroy(int id) {
  WalkerDev &w = walker_ref(id);
  walker_free_bten(w);
  walker_free_mpo(w);
  free_bmps(w.b);
  walkers_.erase(id);
}

template <typename T>
void Engine<T>::walker_info(int id, int *pos, int *stack, int *lcol, int *rcol) {
  WalkerDev &w = walker_ref(id);
  if (pos) *pos = w.pos;
  if (stack) *stack = w.stack;
  if (lcol) *lcol = w.lcol;
  if (rcol) *rcol = w.rcol;
}

// the TransferMPO of the calls that follow
template <typename T>
void Engine<T>::walker_set_mpo(int id, int num, const int32_t *states, const double *tensors, int n_tensors) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  const bool hor = (w.pos == UP || w.pos == DOWN);
  const int N = mps_len(w.pos), lim = hor ? Ly_ : Lx_;
  PG_REQUIRE(num >= 0 && num < lim, 1, "BMPSWalker: MPO slice outside the lattice");
  PG_REQUIRE(!(states && tensors), 1, "BMPSWalker: name the MPO by states OR by tensors");
  PG_REQUIRE(!tensors || n_tensors == 1 || n_tensors == nw_, 1, "BMPSWalker: explicit MPO tensors come as one set or one set per walker");
  // validate and build BEFORE the walker's current MPO is released: a bad argument leaves the walker as it was
  std::vector<int> tab;
  if (states) {
    // a full configuration table with the slice replaced (same layout as the walkers' own table: every kernel's selector works)
    tab = hcfg_;
    for (int wk = 0; wk < nw_; ++wk)
      for (int j = 0; j < N; ++j) {
        const int s = states[(size_t)wk * N + j];
        PG_REQUIRE(s >= 0 && s < dp_, 4, "BMPSWalker: MPO state exceeds the physical dimension");
        const int r = hor ? num : j, c = hor ? j : num;
        tab[(size_t)wk * Ly_ * Lx_ + r * Lx_ + c] = s;
      }
  }
  walker_free_mpo(w);
  w.mpo_num = num;
  if (states) {
    w.mpo_cfg = (int *)arena_.alloc(sizeof(int) * tab.size());
    PG_CHECK_HIP(hipMemcpyAsync(w.mpo_cfg, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    w.mpo_hrow.assign(states, states + (size_t)nw_ * N);
  } else if (tensors) {
    // host [nt][N][L][D][R][U] zero padded to D^4 -> device [N][nt][slot], compact inside the slot (as the SITPS)
    std::vector<T> buf((size_t)N * n_tensors * slot_, T(0));
    for (int j = 0; j < N; ++j) {
      int dd[4];
      site_dims(hor ? num : j, hor ? j : num, dd);
      for (int q = 0; q < n_tensors; ++q) {
        const size_t src0 = ((size_t)q * N + j) * slot_, dst0 = ((size_t)j * n_tensors + q) * slot_;
        size_t o = 0;
        for (int a = 0; a < dd[0]; ++a)
          for (int b = 0; b < dd[1]; ++b)
            for (int c = 0; c < dd[2]; ++c)
              for (int e = 0; e < dd[3]; ++e) {
                const size_t src = src0 + (((size_t)a * D_ + b) * D_ + c) * D_ + e;
                if constexpr (kCplx) {
                  typedef typename real_of<T>::type R;
                  buf[dst0 + o++] = T(R(tensors[2 * src]), R(tensors[2 * src + 1]));
                } else {
                  buf[dst0 + o++] = T(tensors[src]);
                }
              }
      }
    }
    w.mpo_tens = (T *)arena_.alloc(sizeof(T) * buf.size());
    w.mpo_nt = n_tensors;
    PG_CHECK_HIP(hipMemcpyAsync(w.mpo_tens, buf.data(), sizeof(T) * buf.size(), hipMemcpyHostToDevice, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    ensure_iota();
  }
}

// The excited row of the structure-factor mixin (structure_factor_measurement_mixin.h:127-134: the row y1 of the network with the
// tensor of the source site replaced) named without a host table: the walkers' configuration table is copied on the device and the
// one site patched there, state s -> state_map[s]; no upload, no synchronisation.  open_out[w] = the map changes walker w's state
// (from the host mirror).  Afterwards the walker is as after walker_set_mpo(states) with that row.
template <typename T>
void Engine<T>::walker_set_mpo_excited(int id, int num, int col, const int32_t *state_map, uint8_t *open_out) {
  require_ready();
  PG_REQUIRE(state_map, 1, "BMPSWalker: null state map");
  WalkerDev &w = walker_ref(id);
  PG_REQUIRE(w.pos == UP, 1, "BMPSWalker: unsupported direction (the excited row is a row below an UP walker)");
  PG_REQUIRE(num >= 0 && num < Ly_ && col >= 0 && col < Lx_, 1, "BMPSWalker: excited site outside the lattice");
  PG_REQUIRE(dp_ <= WK_MAXDP, 1, "BMPSWalker: state maps serve physical dimensions up to 32");
  require_states(state_map, dp_, dp_, "BMPSWalker: mapped state exceeds the physical dimension");
  WalkerStateMap map{};
  for (int s = 0; s < dp_; ++s) map.v[s] = state_map[s];
  const int N = Lx_, sites = Ly_ * Lx_, site = num * Lx_ + col;
  std::vector<int> hrow((size_t)nw_ * N);
  for (int wk = 0; wk < nw_; ++wk) {
    const int *c = hcfg_.data() + (size_t)wk * sites + (size_t)num * Lx_;
    std::copy(c, c + N, hrow.begin() + (size_t)wk * N);
    hrow[(size_t)wk * N + col] = map.v[c[col]];
    if (open_out) open_out[wk] = map.v[c[col]] != c[col];
  }
  walker_free_mpo(w);
  w.mpo_num = num;
  w.mpo_cfg = (int *)arena_.alloc(sizeof(int) * (size_t)nw_ * sites);
  PG_CHECK_HIP(hipMemcpyAsync(w.mpo_cfg, cfg_, sizeof(int) * (size_t)nw_ * sites, hipMemcpyDeviceToDevice, stream_));
  hipLaunchKernelGGL(walker_excite_site_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, w.mpo_cfg, sites, site, map, nw_);
  PG_CHECK_HIP(hipGetLastError());
  w.mpo_hrow.swap(hrow);
}

// The excited row of the singlet-pair correlation (singlet_pair_correlation_measurement_mixin.h:376-401: the MPO of row y1 with the
// tensors of the reference bond replaced) as walker_set_mpo_excited names its row: the configuration table copied on the device and
// ONE two-site patch, the extended states of the pair derived there; no upload, no synchronisation.  open_out / sign_out [n] from the
// host mirror (nullable).  Afterwards the walker is as after walker_set_mpo(states) with that row.
template <typename T>
void Engine<T>::walker_set_mpo_excited_pair(int id, int num, int col, int d, const int32_t *occ, const int32_t *pair_table, int slot,
                                            uint8_t *open_out, int32_t *sign_out) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  PG_REQUIRE(w.pos == UP, 1, "BMPSWalker: unsupported direction (the excited row is a row below an UP walker)");
  PG_REQUIRE(num >= 0 && num < Ly_ && col >= 0 && col + 1 < Lx_, 1, "BMPSWalker: excited bond outside the row");
  PG_REQUIRE(slot == 0 || slot == 1, 1, "BMPSWalker: pair slot outside {0, 1}");
  WalkerPairMap maps[2] = {};
  const unsigned occ_bits = walker_pair_maps(d, dp_, occ, pair_table, &maps[0], &maps[1]);
  const WalkerPairMap &map = maps[slot];
  const int N = Lx_, sites = Ly_ * Lx_, site = num * Lx_ + col;
  std::vector<int> hrow((size_t)nw_ * N);
  for (int wk = 0; wk < nw_; ++wk) {
    const int *c = hcfg_.data() + (size_t)wk * sites + (size_t)num * Lx_;
    for (int j = 0; j < N; ++j)
      PG_REQUIRE(c[j] / d < 2, 3, "BMPSWalker: extended states of the column-major order in the row (rows: variants 0 / 1)");
    std::copy(c, c + N, hrow.begin() + (size_t)wk * N);
  }
  for (int wk = 0; wk < nw_; ++wk) {
    int *r = hrow.data() + (size_t)wk * N + col;
    int c1, c2;
    const int sg = walker_pair_apply(map, d, occ_bits, r[0], r[1], &c1, &c2);
    r[0] = c1; r[1] = c2;
    if (open_out) open_out[wk] = sg != 0;
    if (sign_out) sign_out[wk] = sg;
  }
  walker_free_mpo(w);
  w.mpo_num = num;
  w.mpo_cfg = (int *)arena_.alloc(sizeof(int) * (size_t)nw_ * sites);
  PG_CHECK_HIP(hipMemcpyAsync(w.mpo_cfg, cfg_, sizeof(int) * (size_t)nw_ * sites, hipMemcpyDeviceToDevice, stream_));
  hipLaunchKernelGGL(walker_excite_pair_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, w.mpo_cfg, sites, site, d, occ_bits, map, nw_);
  PG_CHECK_HIP(hipGetLastError());
  w.mpo_hrow.swap(hrow);
}

template <typename T>
void Engine<T>::ensure_iota() {
  if (iota_) return;
  std::vector<int> h(maxw_ + 1);
  for (int i = 0; i < maxw_; ++i) h[i + 1] = i;
  h[0] = 0;                                   // iota_[0] alone = the selector of a shared tensor set (stride 0)
  iota_ = (int *)arena_.alloc(sizeof(int) * h.size());
  PG_CHECK_HIP(hipMemcpyAsync(iota_, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
}

// scope guard: cfg_site / site selection of slice w.mpo_num follow the walker's MPO while it lives
template <typename T>
struct Engine<T>::MpoScope {
  Engine<T> &e;
  MpoScope(Engine<T> &eng, const WalkerDev &w) : e(eng) {
    PG_REQUIRE(w.mpo_num >= 0, 3, "BMPSWalker: no MPO set (pepsgpu_walker_set_mpo)");
    PG_REQUIRE(!e.cfg_ovr_tab_, 3, "BMPSWalker: a configuration override is set (pepsgpu_cfg_override_slice): clear it first");
    e.ovr_hor_ = (w.pos == UP || w.pos == DOWN);
    e.ovr_num_ = w.mpo_num;
    e.ovr_cfg_ = w.mpo_cfg;
    e.ovr_tens_ = w.mpo_tens;
    e.ovr_nt_ = w.mpo_nt;
    e.ovr_on_ = true;
  }
  ~MpoScope() { e.ovr_on_ = false; e.ovr_cfg_ = nullptr; e.ovr_tens_ = nullptr; }
};

template <typename T>
typename Engine<T>::BMPSDev Engine<T>::absorb_any(int pos, int num, const BMPSDev &in) {
  if constexpr (kCplx) {
    if (scheme_ != 0 && mps_len(pos) > 2) return absorb_variational(pos, num, in);
    return absorb_simple(pos, num, in);
  } else {
    if (scheme_ != 0 && mps_len(pos) > 2) return absorb_variational(pos, num, in);
    return absorb_svd(pos, num, in);
  }
}

// Evolve(mpo) (bmps_walker.h:13-21): the stack-size counter is NOT advanced
template <typename T>
void Engine<T>::walker_evolve(int id) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  MpoScope scope(*this, w);
  // (the routing hints of absorb_svd are keyed by (pos, num): a foreign MPO must not teach them anything about the network's row)
  const char keep = redo_seen_[w.pos][w.mpo_num];
  BMPSDev out;
  try { out = absorb_any(w.pos, w.mpo_num, w.b); } catch (...) { redo_seen_[w.pos][w.mpo_num] = keep; throw; }
  redo_seen_[w.pos][w.mpo_num] = keep;
  free_bmps(w.b);
  w.b = std::move(out);
  walker_free_bten(w);
}

// EvolveStep (bmps_walker.h:23-49)
template <typename T>
void Engine<T>::walker_evolve_step(int id) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  PG_REQUIRE(w.stack > 0, 3, "BMPSWalker::EvolveStep: empty walker");
  int num;
  if (w.pos == UP || w.pos == LEFT) num = w.stack - 1;
  else if (w.pos == DOWN) num = Ly_ - w.stack;
  else num = Lx_ - w.stack;
  if (w.pos == UP && num >= Ly_ - 1) return;
  if (w.pos == LEFT && num >= Lx_ - 1) return;
  PG_REQUIRE(num >= 0, 3, "BMPSWalker::EvolveStep: no slice left to absorb");
  BMPSDev out = absorb_any(w.pos, num, w.b);
  free_bmps(w.b);
  w.b = std::move(out);
  w.stack++;
  walker_free_bten(w);
}

template <typename T>
const typename Engine<T>::BMPSDev &Engine<T>::walker_opposite(const WalkerDev &w, int opp_level, const char *what) {
  PG_REQUIRE(w.pos == UP, 1, "BMPSWalker: unsupported direction pair (walker must be UP, opposite must be DOWN)");
  PG_REQUIRE(opp_level >= 0 && opp_level < bmps_size(DOWN), 3, "BMPSWalker: opposite boundary not available (DOWN stack level)");
  (void)what;
  return bmps_[DOWN][opp_level];
}

template <typename T>
void Engine<T>::walker_grow_left(WalkerDev &w, const BMPSDev &opp) {
  const int N = Lx_;
  if (w.btl.empty()) {
    PG_REQUIRE(w.lcol == 0, 3, "BMPSWalker::GrowBTenLeftStep: bten_left_ is empty but col != 0");
    BTenDev v; v.t = ones3(); v.logscale = zeros_f64();
    w.btl.push_back(v);
  }
  PG_REQUIRE(w.lcol < N, 3, "BMPSWalker::GrowBTenLeftStep: Cannot grow beyond N.");
  const int col = w.lcol, j1 = N - 1 - col;
  auto lv = [](const BMPSDev &b, int j) -> const int * { return (int)b.live.size() > j ? b.live[j] : nullptr; };
  BTenDev nb = bten_step(LEFT, w.btl.back(), w.b.t[j1], cfg_site(w.mpo_num, col), opp.t[col], 1, true, 1, lv(w.b, j1), lv(w.b, j1 + 1),
                         lv(opp, col), lv(opp, col + 1));
  w.btl.push_back(nb);
  w.lcol++;
}

template <typename T>
void Engine<T>::walker_grow_right(WalkerDev &w, const BMPSDev &opp) {
  const int N = Lx_;
  PG_REQUIRE(!w.btr.empty(), 3, "BMPSWalker::GrowBTenRightStep: Right BTen cache is empty. Call InitBTenRight first.");
  PG_REQUIRE(w.rcol > 0, 3, "BMPSWalker::GrowBTenRightStep: Cannot grow further left. col is already 0.");
  const int col = w.rcol - 1, j2 = N - 1 - col;
  auto lv = [](const BMPSDev &b, int j) -> const int * { return (int)b.live.size() > j ? b.live[j] : nullptr; };
  BTenDev nb = bten_step(RIGHT, w.btr.back(), opp.t[col], cfg_site(w.mpo_num, col), w.b.t[j2], 1, true, 1, lv(opp, col), lv(opp, col + 1),
                         lv(w.b, j2), lv(w.b, j2 + 1));
  w.btr.push_back(nb);
  w.rcol--;
}

template <typename T>
void Engine<T>::walker_init_bten(int id, int opp_level, int side, int target_col) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  const BMPSDev &opp = walker_opposite(w, opp_level, "InitBTen");
  MpoScope scope(*this, w);
  walker_init_side(w, opp, side, target_col);
}

// InitBTenLeft / InitBTenRight (bmps_walker.h:216-272) under the MpoScope of the caller
template <typename T>
void Engine<T>::walker_init_side(WalkerDev &w, const BMPSDev &opp, int side, int target_col) {
  PG_REQUIRE(target_col >= 0, 1, "BMPSWalker::InitBTen: negative column");
  const int N = Lx_;
  if (side == LEFT) {
    for (auto &b : w.btl) { arena_.free(b.t.p); arena_.free(b.logscale); }
    w.btl.clear(); w.lcol = 0;
    BTenDev v; v.t = ones3(); v.logscale = zeros_f64();
    w.btl.push_back(v);
    while (w.lcol < target_col && w.lcol < N) walker_grow_left(w, opp);
  } else {
    PG_REQUIRE(side == RIGHT, 1, "BMPSWalker::InitBTen: position must be LEFT or RIGHT");
    for (auto &b : w.btr) { arena_.free(b.t.p); arena_.free(b.logscale); }
    w.btr.clear(); w.rcol = N;
    BTenDev v; v.t = ones3(); v.logscale = zeros_f64();
    w.btr.push_back(v);
    while (w.rcol > target_col + 1 && w.rcol > 0) walker_grow_right(w, opp);
  }
}

template <typename T>
void Engine<T>::walker_grow_bten_step(int id, int opp_level, int side) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  const BMPSDev &opp = walker_opposite(w, opp_level, "GrowBTenStep");
  MpoScope scope(*this, w);
  if (side == LEFT) walker_grow_left(w, opp);
  else { PG_REQUIRE(side == RIGHT, 1, "BMPSWalker: position must be LEFT or RIGHT"); walker_grow_right(w, opp); }
}

// ShiftBTenWindow (bmps_walker.h:326-350)
template <typename T>
void Engine<T>::walker_shift_bten_window(int id, int opp_level, int side) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  const BMPSDev &opp = walker_opposite(w, opp_level, "ShiftBTenWindow");
  MpoScope scope(*this, w);
  if (side == LEFT) {
    PG_REQUIRE(!w.btl.empty(), 3, "BMPSWalker::ShiftBTenWindow: Left BTen cache is empty.");
    PG_REQUIRE(!w.btr.empty(), 3, "BMPSWalker::GrowBTenRightStep: Right BTen cache is empty. Call InitBTenRight first.");
    arena_.free(w.btl.back().t.p); arena_.free(w.btl.back().logscale);
    w.btl.pop_back(); w.lcol--;
    walker_grow_right(w, opp);
  } else {
    PG_REQUIRE(side == RIGHT, 1, "BMPSWalker: position must be LEFT or RIGHT");
    PG_REQUIRE(!w.btr.empty(), 3, "BMPSWalker::ShiftBTenWindow: Right BTen cache is empty.");
    arena_.free(w.btr.back().t.p); arena_.free(w.btr.back().logscale);
    w.btr.pop_back(); w.rcol++;
    walker_grow_left(w, opp);
  }
}

// the replacement site of a trace: the MPO's own tensor (nothing given), a component of the SITPS per walker (states), or an
// explicit tensor (one shared or one per walker, host layout [nt][L][D][R][U] padded)
template <typename T>
typename Engine<T>::SiteSel Engine<T>::walker_site(const WalkerDev &w, int col, const int32_t *states, int sstride, const double *tensor,
                                                   int n_tensors, long tstride, std::vector<void *> &tmp) {
  if (!states && !tensor) return cfg_site(w.mpo_num, col);
  if (states) {
    std::vector<int> h(nw_);
    for (int k = 0; k < nw_; ++k) {
      h[k] = states[(size_t)k * sstride];
      PG_REQUIRE(h[k] >= 0 && h[k] < dp_, 4, "BMPSWalker: replacement state exceeds the physical dimension");
    }
    int *d = (int *)arena_.alloc(sizeof(int) * nw_);
    tmp.push_back(d);
    PG_CHECK_HIP(hipMemcpyAsync(d, h.data(), sizeof(int) * nw_, hipMemcpyHostToDevice, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    SiteSel s{w.mpo_num, col, d, 1};
    s.base = sitps_ + (long)(w.mpo_num * Lx_ + col) * dp_ * slot_;     // the SITPS itself, whatever the MPO is made of
    return s;
  }
  PG_REQUIRE(n_tensors == 1 || n_tensors == nw_, 1, "BMPSWalker: a replacement tensor comes once or once per walker");
  int dd[4];
  site_dims(w.mpo_num, col, dd);
  std::vector<T> buf((size_t)n_tensors * slot_, T(0));
  for (int q = 0; q < n_tensors; ++q) {
    size_t o = 0;
    for (int a = 0; a < dd[0]; ++a)
      for (int b = 0; b < dd[1]; ++b)
        for (int c = 0; c < dd[2]; ++c)
          for (int e = 0; e < dd[3]; ++e) {
            const size_t src = (size_t)q * tstride + (((size_t)a * D_ + b) * D_ + c) * D_ + e;
            if constexpr (kCplx) {
              typedef typename real_of<T>::type R;
              buf[(size_t)q * slot_ + o++] = T(R(tensor[2 * src]), R(tensor[2 * src + 1]));
            } else {
              buf[(size_t)q * slot_ + o++] = T(tensor[src]);
            }
          }
  }
  T *d = (T *)arena_.alloc(sizeof(T) * buf.size());
  tmp.push_back(d);
  PG_CHECK_HIP(hipMemcpyAsync(d, buf.data(), sizeof(T) * buf.size(), hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  ensure_iota();
  SiteSel s{w.mpo_num, col, n_tensors == 1 ? iota_ : iota_ + 1, n_tensors == 1 ? 0 : 1};
  s.base = d;
  return s;
}

// TraceWithBTen (bmps_walker.h:352-392) / TraceWithTwoSiteBTen (:394-463); two_site: states = [n][2], tensors = [nt][2][D^4]
template <typename T>
void Engine<T>::walker_trace(int id, int opp_level, int site_col, int two_site, const int32_t *states, const double *tensors, int n_tensors,
                             double *out) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  const BMPSDev &opp = walker_opposite(w, opp_level, "TraceWithBTen");
  MpoScope scope(*this, w);
  ArenaScope ascope(arena_);
  const int N = Lx_;
  PG_REQUIRE(site_col >= 0 && site_col + (two_site ? 1 : 0) < N, 1, "BMPSWalker::TraceWithBTen: site column out of bounds");
  PG_REQUIRE(!w.btl.empty() && !w.btr.empty(), 3, "BMPSWalker::TraceWithBTen: BTen caches not initialized.");
  PG_REQUIRE(w.lcol >= site_col, 3, "BMPSWalker::TraceWithBTen: Left BTen insufficient.");
  const int last = site_col + (two_site ? 1 : 0);
  PG_REQUIRE(w.rcol <= last + 1, 3, "BMPSWalker::TraceWithBTen: Right BTen insufficient.");
  const int right_idx = N - 1 - last;
  PG_REQUIRE(site_col < (int)w.btl.size() && right_idx < (int)w.btr.size(), 3, "BMPSWalker::TraceWithBTen: BTen index out of bounds.");
  std::vector<void *> tmp;
  const int ns = two_site ? 2 : 1;
  auto lv = [](const BMPSDev &b, int j) -> const int * { return (int)b.live.size() > j ? b.live[j] : nullptr; };
  const BTenDev &lb = w.btl[site_col], &rb = w.btr[right_idx];
  SiteSel sa = walker_site(w, site_col, states, ns, tensors, n_tensors, (long)ns * slot_, tmp);
  const int ja = N - 1 - site_col;
  BTenDev t2 = bten_step(LEFT, lb, w.b.t[ja], sa, opp.t[site_col], 1, false, 1, lv(w.b, ja), lv(w.b, ja + 1), lv(opp, site_col),
                         lv(opp, site_col + 1));
  if (two_site) {
    SiteSel sb = walker_site(w, site_col + 1, states ? states + 1 : nullptr, ns, tensors ? tensors + slot_ * kOut : nullptr, n_tensors,
                             (long)ns * slot_, tmp);
    const int jb = N - 2 - site_col;
    BTenDev t3 = bten_step(LEFT, t2, w.b.t[jb], sb, opp.t[site_col + 1], 1, false, 1, lv(w.b, jb), lv(w.b, jb + 1), lv(opp, site_col + 1),
                           lv(opp, site_col + 2));
    free_ten(t2.t);
    t2 = t3;
  }
  double *lsum = zeros_f64();
  add_logs(lsum, w.b.logscale, opp.logscale, lb.logscale, rb.logscale);
  finish_dot(t2.t, 1, rb.t, 1, 1, lsum, out);
  free_ten(t2.t);
  arena_.free(lsum);
  for (void *p : tmp) arena_.free(p);
}

// The body of the structure-factor mixin's target-row loop (structure_factor_measurement_mixin.h:160-194) in one call:
// InitBTenLeft(opp, N), InitBTenRight(opp, N - 1), then for x2 = N - 1 .. 0 TraceWithBTen at x2 with the site's state s replaced by
// site_map[s] and GrowBTenRightStep while x2 > 0 -- the launches of the per-call sequence in its order, candidates and skip flags
// built on the device, the values collected in a table on the device, ONE read-back.  out [n][N]: the trace where walker_mask[w] != 0
// (NULL: every walker) and site_map[s] != s, exactly 0.0 elsewhere (those walkers are skipped inside the contraction, bten_step's
// `skip`; a position at which the host mirror shows no open walker makes no trace launch at all).
template <typename T>
void Engine<T>::walker_trace_slice(int id, int opp_level, const int32_t *site_map, const uint8_t *walker_mask, double *out) {
  require_ready();
  PG_REQUIRE(site_map && out, 1, "BMPSWalker::TraceSlice: null buffer");
  WalkerDev &w = walker_ref(id);
  const BMPSDev &opp = walker_opposite(w, opp_level, "TraceSlice");
  PG_REQUIRE(dp_ <= WK_MAXDP, 1, "BMPSWalker: state maps serve physical dimensions up to 32");
  require_states(site_map, dp_, dp_, "BMPSWalker: mapped state exceeds the physical dimension");
  PG_REQUIRE(w.mpo_num < 0 || !w.mpo_tens, 3, "BMPSWalker::TraceSlice: the MPO is given as explicit tensors (it has no state to map)");
  MpoScope scope(*this, w);                  // (no MPO set, configuration override: status 3 before anything is released)
  const int N = Lx_, sites = Ly_ * Lx_;
  WalkerStateMap map{};
  for (int s = 0; s < dp_; ++s) map.v[s] = site_map[s];
  // the MPO's states along the row as the host knows them: its mirror, or the walkers' own configurations
  const bool mirrored = !w.mpo_cfg || !w.mpo_hrow.empty();
  auto hstate = [&](int wk, int x) {
    return w.mpo_cfg ? w.mpo_hrow[(size_t)wk * N + x] : hcfg_[(size_t)wk * sites + (size_t)w.mpo_num * Lx_ + x];
  };
  const int *dstates = w.mpo_cfg ? w.mpo_cfg : cfg_;
  std::vector<int> hmask;
  if (walker_mask) hmask.assign(walker_mask, walker_mask + nw_);
  ArenaBuf<int> dmask(arena_, walker_mask ? (size_t)nw_ : 0);
  if (dmask) PG_CHECK_HIP(hipMemcpyAsync(dmask, hmask.data(), sizeof(int) * nw_, hipMemcpyHostToDevice, stream_));
  ArenaBuf<double> dval(arena_, kOut * (size_t)nw_ * N);                  // value table [n][N] of Acc scalars, zero = closed
  PG_CHECK_HIP(hipMemsetAsync(dval, 0, sizeof(double) * kOut * (size_t)nw_ * N, stream_));
  ArenaBuf<int> dcand(arena_, 2 * (size_t)nw_);                           // replacement state [n], skip flag [n]
  int *dskip = dcand + nw_;
  walker_init_side(w, opp, LEFT, N);
  walker_init_side(w, opp, RIGHT, N - 1);
  auto lv = [](const BMPSDev &b, int j) -> const int * { return (int)b.live.size() > j ? b.live[j] : nullptr; };
  for (int x2 = N - 1; x2 >= 0; --x2) {
    bool any = !mirrored;
    for (int wk = 0; wk < nw_ && !any; ++wk) {
      const int s = hstate(wk, x2);
      any = map.v[s] != s && (!walker_mask || walker_mask[wk]);
    }
    if (any) {
      ArenaScope ascope(arena_);               // (the temporaries of this trace; the caches grow outside it)
      hipLaunchKernelGGL(walker_trace_cand_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, dstates, sites, w.mpo_num * Lx_ + x2, map,
                         (const int *)dmask, (int *)dcand, dskip, nw_);
      PG_CHECK_HIP(hipGetLastError());
      SiteSel sa{w.mpo_num, x2, dcand, 1};
      sa.base = sitps_ + (long)(w.mpo_num * Lx_ + x2) * dp_ * slot_;
      const int ja = N - 1 - x2;
      const BTenDev &lb = w.btl[x2], &rb = w.btr[N - 1 - x2];
      BTenDev t2 = bten_step(LEFT, lb, w.b.t[ja], sa, opp.t[x2], 1, false, 1, lv(w.b, ja), lv(w.b, ja + 1), lv(opp, x2), lv(opp, x2 + 1),
                             dskip);
      double *lsum = zeros_f64();
      add_logs(lsum, w.b.logscale, opp.logscale, lb.logscale, rb.logscale);
      Acc *res = finish_dot_device(t2.t, 1, rb.t, 1, 1);
      // (a skipped walker keeps the zero its entry holds: `same` copies column x2 onto itself)
      hipLaunchKernelGGL(slice_store_value_kernel<Acc>, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, (const Acc *)res,
                         (const double *)lsum, (double *)dval, N, x2, 1, (const int *)dskip, x2, nw_);
      PG_CHECK_HIP(hipGetLastError());
      free_ten(t2.t);
      arena_.free(res); arena_.free(lsum);
    }
    if (x2 > 0) walker_grow_right(w, opp);
  }
  PG_CHECK_HIP(hipMemcpyAsync(out, dval, sizeof(double) * kOut * (size_t)nw_ * N, hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  walker_slice_calls() += 1;
}

// The target-row loop of the singlet-pair correlation (singlet_pair_correlation_measurement_mixin.h:446-519 on bmps_walker.h:216-463)
// in one call: InitBTenLeft(opp, 0), InitBTenRight(opp, 1), then for x2 = 0 .. N - 2 TraceWithTwoSiteBTen at x2 with the states of
// (x2, x2 + 1) replaced by candidate k of the pair table, k = 0, 1, and ShiftBTenWindow(RIGHT) while x2 < N - 2.  Each slot is the
// two half steps and the dot of walker_trace, one candidate per walker -- the launches of the per-call sequence in its order, so the
// f32 steps stay on the chained kernels and the numbers are the per-call path's; a slot for which the host mirror shows no open walker
// (for the measurement: slot 1 always) launches nothing.  out [n][N - 1][2] = sign trace exp(log scales), exactly 0.0 for "no
// candidate" and for masked walkers.  The caches end as the per-call sequence leaves them: lcol = N - 2, rcol = N (N >= 2).
template <typename T>
void Engine<T>::walker_pair_trace_slice(int id, int opp_level, int d, const int32_t *occ, const int32_t *pair_table,
                                        const uint8_t *walker_mask, double *out) {
  require_ready();
  PG_REQUIRE(out, 1, "BMPSWalker::PairTraceSlice: null buffer");
  WalkerDev &w = walker_ref(id);
  WalkerPairMap maps[2] = {};
  const unsigned occ_bits = walker_pair_maps(d, dp_, occ, pair_table, &maps[0], &maps[1]);
  const BMPSDev &opp = walker_opposite(w, opp_level, "PairTraceSlice");
  PG_REQUIRE(w.mpo_num < 0 || !w.mpo_tens, 3, "BMPSWalker::PairTraceSlice: the MPO is given as explicit tensors (it has no state to map)");
  MpoScope scope(*this, w);                  // (no MPO set, configuration override: status 3 before anything is released)
  const int N = Lx_, sites = Ly_ * Lx_, np = N - 1;
  PG_REQUIRE(N >= 2, 1, "BMPSWalker::PairTraceSlice: a row of one site has no bond");
  const bool mirrored = !w.mpo_cfg || !w.mpo_hrow.empty();
  PG_REQUIRE(mirrored, 3, "BMPSWalker::PairTraceSlice: the MPO's states are not mirrored on the host");
  auto hstate = [&](int wk, int x) {
    return w.mpo_cfg ? w.mpo_hrow[(size_t)wk * N + x] : hcfg_[(size_t)wk * sites + (size_t)w.mpo_num * Lx_ + x];
  };
  for (int wk = 0; wk < nw_; ++wk)
    for (int x = 0; x < N; ++x)
      PG_REQUIRE(hstate(wk, x) / d < 2, 3, "BMPSWalker: extended states of the column-major order in the row (rows: variants 0 / 1)");
  const int *dstates = w.mpo_cfg ? w.mpo_cfg : cfg_;
  std::vector<int> hmask;
  if (walker_mask) hmask.assign(walker_mask, walker_mask + nw_);
  ArenaBuf<int> dmask(arena_, walker_mask ? (size_t)nw_ : 0);
  if (dmask) PG_CHECK_HIP(hipMemcpyAsync(dmask, hmask.data(), sizeof(int) * nw_, hipMemcpyHostToDevice, stream_));
  const size_t nval = kOut * (size_t)nw_ * np * 2;
  ArenaBuf<double> dval(arena_, nval);                                    // value table [n][N - 1][2] of Acc scalars, zero = closed
  PG_CHECK_HIP(hipMemsetAsync(dval, 0, sizeof(double) * nval, stream_));
  ArenaBuf<int> dcand(arena_, 8 * (size_t)nw_);                           // candidates [n][2][2], skip [2][n], sign [n][2]
  int *dskip = dcand + 4 * (size_t)nw_, *dsign = dskip + 2 * (size_t)nw_;
  walker_init_side(w, opp, LEFT, 0);
  walker_init_side(w, opp, RIGHT, 1);
  auto lv = [](const BMPSDev &b, int j) -> const int * { return (int)b.live.size() > j ? b.live[j] : nullptr; };
  const int gb = (nw_ + 255) / 256;
  for (int x2 = 0; x2 < np; ++x2) {
    bool any[2] = {false, false};
    for (int k = 0; k < 2; ++k)
      for (int wk = 0; wk < nw_ && !any[k]; ++wk) {
        if (walker_mask && !walker_mask[wk]) continue;
        int c1, c2;
        any[k] = walker_pair_apply(maps[k], d, occ_bits, hstate(wk, x2), hstate(wk, x2 + 1), &c1, &c2) != 0;
      }
    if (any[0] || any[1]) {
      hipLaunchKernelGGL(walker_pair_cand_kernel, dim3(gb), dim3(256), 0, stream_, dstates, sites, w.mpo_num * Lx_ + x2, d, occ_bits, maps[0],
                         maps[1], (const int *)dmask, (int *)dcand, dskip, dsign, nw_);
      PG_CHECK_HIP(hipGetLastError());
    }
    for (int k = 0; k < 2; ++k) {
      if (!any[k]) continue;
      ArenaScope ascope(arena_);               // (the temporaries of this trace; the caches grow outside it)
      const int *skip = dskip + (size_t)k * nw_;
      SiteSel sa{w.mpo_num, x2, dcand + 2 * k, 4}, sb{w.mpo_num, x2 + 1, dcand + 2 * k + 1, 4};
      sa.base = sitps_ + (long)(w.mpo_num * Lx_ + x2) * dp_ * slot_;
      sb.base = sitps_ + (long)(w.mpo_num * Lx_ + x2 + 1) * dp_ * slot_;
      const int ja = N - 1 - x2, jb = N - 2 - x2;
      const BTenDev &lb = w.btl[x2], &rb = w.btr[N - 2 - x2];
      BTenDev t2 = bten_step(LEFT, lb, w.b.t[ja], sa, opp.t[x2], 1, false, 1, lv(w.b, ja), lv(w.b, ja + 1), lv(opp, x2), lv(opp, x2 + 1),
                             skip);
      BTenDev t3 = bten_step(LEFT, t2, w.b.t[jb], sb, opp.t[x2 + 1], 1, false, 1, lv(w.b, jb), lv(w.b, jb + 1), lv(opp, x2 + 1),
                             lv(opp, x2 + 2), skip);
      free_ten(t2.t);
      double *lsum = zeros_f64();
      add_logs(lsum, w.b.logscale, opp.logscale, lb.logscale, rb.logscale);
      Acc *res = finish_dot_device(t3.t, 1, rb.t, 1, 1);
      hipLaunchKernelGGL(walker_pair_store_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, (const Acc *)res, (const double *)lsum,
                         (const int *)dsign + k, 2, skip, (double *)dval, 2 * np, 2 * x2 + k, nw_);
      PG_CHECK_HIP(hipGetLastError());
      free_ten(t3.t);
      arena_.free(res); arena_.free(lsum);
    }
    if (x2 < np - 1) {                         // ShiftBTenWindow(RIGHT)
      arena_.free(w.btr.back().t.p); arena_.free(w.btr.back().logscale);
      w.btr.pop_back(); w.rcol++;
      walker_grow_left(w, opp);
    }
  }
  PG_CHECK_HIP(hipMemcpyAsync(out, dval, sizeof(double) * nval, hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  walker_pair_slice_calls() += 1;
}

// ContractRow (bmps_walker.h:60-214): <walker | mpo | opposite>.  The reference multiplies the columns right to left into a
// six-leg accumulator; the value is the same closed network the BTen route contracts (its own tests assert exactly that,
// test_bmps_contractor.cpp:1233-1274), so it is computed as LEFT environment over the first N - 1 columns, vacuum on the right,
// trace at the last column -- without touching the walker's caches.
template <typename T>
void Engine<T>::walker_contract_row(int id, int opp_level, double *out) {
  require_ready();
  WalkerDev &w = walker_ref(id);
  (void)walker_opposite(w, opp_level, "ContractRow");
  std::vector<BTenDev> kl, kr;
  kl.swap(w.btl); kr.swap(w.btr);
  const int lc = w.lcol, rc = w.rcol;
  w.lcol = 0; w.rcol = 0;
  auto restore = [&]() {
    walker_free_bten(w);
    w.btl.swap(kl); w.btr.swap(kr);
    w.lcol = lc; w.rcol = rc;
  };
  try {
    walker_init_bten(id, opp_level, LEFT, Lx_ - 1);
    walker_init_bten(id, opp_level, RIGHT, Lx_ - 1);
    walker_trace(id, opp_level, Lx_ - 1, 0, nullptr, nullptr, 0, out);
  } catch (...) { restore(); throw; }
  restore();
}

template <typename T>
void Engine<T>::walker_clear_bten(int id) { walker_free_bten(walker_ref(id)); }

template <typename T>
void Engine<T>::walker_get_tensor(int id, int idx, int *dims, double *out, double *logscale) {
  WalkerDev &w = walker_ref(id);
  PG_REQUIRE(idx >= 0 && idx < (int)w.b.t.size(), 1, "BMPS tensor index out of range");
  const DTen<T> &t = w.b.t[idx];
  dims[0] = t.d[0]; dims[1] = t.d[1]; dims[2] = t.d[2];
  if (out) {
    std::vector<T> h((size_t)t.n * nw_);
    PG_CHECK_HIP(hipMemcpyAsync(h.data(), t.p, h.size() * sizeof(T), hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < h.size(); ++i) {
      if constexpr (kCplx) { out[2 * i] = (double)h[i].re; out[2 * i + 1] = (double)h[i].im; }
      else out[i] = (double)h[i];
    }
  }
  if (logscale) {
    PG_CHECK_HIP(hipMemcpyAsync(logscale, w.b.logscale, nw_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
  }
}

}  // namespace pepsgpu
