// qlpeps_gpu.h -- C++ host layer above the pepsgpu C ABI, mirroring the reference's operator /
// plugin surface for the boundary-MPS hot path (same names, argument meaning, error behaviour),
// batched over the walkers of one GPU.  Header-only, like the reference.
//
//   reference (one walker per MPI rank)                       here (n walkers per context)
//   BMPSTruncateParams           bmps.h:47-98                 qlpeps_gpu::BMPSTruncateParams
//   Configuration                configuration.h:57           qlpeps_gpu::Configuration
//   SplitIndexTPS                split_index_tps.h:80-606     qlpeps_gpu::SplitIndexTPS (dense, real)
//   BMPSContractor               bmps_contractor.h:187-1027   qlpeps_gpu::BMPSContractor
//   TPSWaveFunctionComponent     wave_function_component.h:136-379   qlpeps_gpu::TPSWaveFunctionComponent
//   MCUpdateSquareNN*OBC         square_nn_updater.h:25-293   qlpeps_gpu::MCUpdateSquareNN*OBC (CRTP)
//   SuwaTodoStateUpdate          suwa_todo_update.h:53-112    qlpeps_gpu::SuwaTodoStateUpdate
//   SquareNNNModelEnergySolver   square_nnn_energy_solver.h   qlpeps_gpu::SquareNNNModelEnergySolver<Model, has_nnn> (CRTP)
//   SquareNNModelEnergySolver    square_nn_energy_solver.h:25 alias with has_nnn_interaction = false
//   SquareSpinOneHalfXXZModelOBC square_spin_onehalf_xxz_obc.h:64-190
//   SquareSpinOneHalfJ1J2XXZModelOBC square_spin_onehalf_j1j2_xxz_obc.h:25-40 (NNN pass on BTen2)
//   SplitIndexTPS::Load / Dump   split_index_tps_impl.h:300-437 (byte-identical .qlten files)
//   Configuration Load / Dump    configuration.h:284-330, :446-464
//   TransverseFieldIsingSquareOBC transverse_field_ising_square_obc.h:28-247
//   ExactSumEnergyEvaluatorMPI   exact_summation_energy_evaluator.h:173-302
//   MCEnergyGradEvaluator accumulation  mc_energy_grad_evaluator.h:245-310
//   SGDParams / AdaGradParams / AdamParams / StochasticReconfigurationParams / OptimizerParams   optimizer/optimizer_params.h
//   ConstantLR / ExponentialDecayLR / StepLR   optimizer/lr_schedulers.h:40-103
//   Optimizer                    optimizer/optimizer.h, optimizer_impl.h (first-order rules and the one-rank SR step, on device buffers)
//   EMATracker / SpikeSignal / SpikeAction / SpikeEventRecord / SpikeStatistics   optimizer/spike_detection.h
//   SpikeRecoveryParams / CheckpointParams / InitialStepSelectorParams / PeriodicStepSelectorParams   optimizer/optimizer_params.h:155-313
//
// Error codes of the ABI are re-raised as the reference's exception types.
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdint>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <random>
#include <sstream>
#include <stdexcept>
#include <optional>
#include <string>
#include <variant>
#include <vector>

#include "../../include/pepsgpu.h"

namespace qlpeps_gpu {

enum BondOrientation { HORIZONTAL = 0, VERTICAL = 1 };      // basic.h:19-22
enum BMPSPOSITION { LEFT = 0, DOWN = 1, RIGHT = 2, UP = 3 };  // basic.h:58-63
enum DIAGONAL_DIR { LEFTUP_TO_RIGHTDOWN = 0, LEFTDOWN_TO_RIGHTUP = 1 };  // basic.h:89-92
using BTenPOSITION = BMPSPOSITION;
enum class CompressMPSScheme { SVD_COMPRESS = 0, VARIATION2Site = 1, VARIATION1Site = 2 };   // bmps.h:31-35

// Element type of the tensors (TenElemT of the reference: QLTEN_Double / QLTEN_Complex; every hot-path test of the reference
// is compiled for both, tests/CMakeLists.txt:57-100).  The classes below that carry tensor elements or amplitudes are
// templates over it (SplitIndexTPST, BMPSContractorT, TPSWaveFunctionComponentT, EnergyAndHolesT, GradAccumulatorT); the
// un-suffixed names are the QLTEN_Double instantiations.  Updaters, solvers and evaluators deduce it from their arguments,
// as the reference's CRTP hooks do (CalEnergyAndHolesImpl<TenElemT, QNT, calchols>, model_energy_solver.h:86-87).
using QLTEN_Double = double;
using QLTEN_Complex = std::complex<double>;
template <typename TenElemT> struct ElemTraits;
template <> struct ElemTraits<double> {
  static constexpr bool is_complex = false;
  static constexpr int host_dtype = PEPSGPU_F64;       // dtype code of a host buffer of this type (pepsgpu_state_upload)
  static int ctx_dtype(int requested) { return requested; }   // PEPSGPU_F32 / PEPSGPU_F64 device tensors
};
template <> struct ElemTraits<std::complex<double>> {
  static constexpr bool is_complex = true;
  static constexpr int host_dtype = PEPSGPU_C128;
  static int ctx_dtype(int) { return PEPSGPU_C128; }
};
inline double ComplexConjugate(double x) { return x; }                                   // qlten ComplexConjugate
inline std::complex<double> ComplexConjugate(const std::complex<double> &x) { return std::conj(x); }
inline double AbsSquare(double x) { return x * x; }
inline double AbsSquare(const std::complex<double> &x) { return std::norm(x); }
// every scalar / tensor the C ABI returns for a complex context is an interleaved (re, im) pair = the layout of std::complex
inline double *dptr(double *p) { return p; }
inline const double *dptr(const double *p) { return p; }
inline double *dptr(std::complex<double> *p) { return reinterpret_cast<double *>(p); }
inline const double *dptr(const std::complex<double> *p) { return reinterpret_cast<const double *>(p); }

struct SiteIdx {                                             // framework/site_idx.h:20-26
  size_t r = 0, c = 0;
  size_t row() const { return r; }
  size_t col() const { return c; }
};

struct BMPSTruncateParams {                                  // bmps.h:47-98
  size_t D_min = 1, D_max = 1;
  double trunc_err = 0.0;
  CompressMPSScheme compress_scheme = CompressMPSScheme::SVD_COMPRESS;
  std::optional<double> convergence_tol;                     // variational schemes only (bmps.h:55-56)
  std::optional<size_t> iter_max;
  static BMPSTruncateParams SVD(size_t d_min, size_t d_max, double trunc_error) {
    BMPSTruncateParams p;
    p.D_min = d_min; p.D_max = d_max; p.trunc_err = trunc_error;
    return p;
  }
  static BMPSTruncateParams Variational2Site(size_t d_min, size_t d_max, double trunc_error, double tol, size_t iters) {
    BMPSTruncateParams p = SVD(d_min, d_max, trunc_error);   // bmps.h:81-88
    p.compress_scheme = CompressMPSScheme::VARIATION2Site; p.convergence_tol = tol; p.iter_max = iters;
    return p;
  }
  static BMPSTruncateParams Variational1Site(size_t d_min, size_t d_max, double trunc_error, double tol, size_t iters) {
    BMPSTruncateParams p = SVD(d_min, d_max, trunc_error);   // bmps.h:90-97
    p.compress_scheme = CompressMPSScheme::VARIATION1Site; p.convergence_tol = tol; p.iter_max = iters;
    return p;
  }
};

inline void check_rc(int rc, pepsgpu_ctx *ctx) {
  if (rc == PEPSGPU_OK) return;
  std::string msg = pepsgpu_last_error(ctx);
  switch (rc) {
    case PEPSGPU_EINVAL: throw std::invalid_argument(msg);
    case PEPSGPU_ESTATE: throw std::logic_error(msg);
    case PEPSGPU_ERANGE: throw std::out_of_range(msg);
    default: throw std::runtime_error(msg);
  }
}

// Walker batch of configurations (configuration.h:57): config(w, site)
class Configuration {
 public:
  Configuration() = default;
  Configuration(size_t n, size_t rows, size_t cols) : n_(n), rows_(rows), cols_(cols), v_(n * rows * cols, 0) {}
  size_t walkers() const { return n_; }
  size_t rows() const { return rows_; }
  size_t cols() const { return cols_; }
  int32_t &operator()(size_t w, const SiteIdx &s) { return v_[(w * rows_ + s.r) * cols_ + s.c]; }
  int32_t operator()(size_t w, const SiteIdx &s) const { return v_[(w * rows_ + s.r) * cols_ + s.c]; }
  const int32_t *data() const { return v_.data(); }
  int32_t *data() { return v_.data(); }

 private:
  size_t n_ = 0, rows_ = 0, cols_ = 0;
  std::vector<int32_t> v_;
};

// Dense SplitIndexTPS<TenElemT, TrivialRepQN> in the ABI upload layout [row][col][s][L][D][R][U], legs zero padded to D.
template <typename TenElemT>
class SplitIndexTPST {
 public:
  SplitIndexTPST() = default;
  SplitIndexTPST(size_t rows, size_t cols, size_t phys_dim, size_t D)
      : rows_(rows), cols_(cols), d_(phys_dim), D_(D), v_(rows * cols * phys_dim * D * D * D * D, TenElemT(0.0)) {}
  size_t rows() const { return rows_; }
  size_t cols() const { return cols_; }
  size_t PhysicalDim() const { return d_; }
  size_t D() const { return D_; }
  size_t slot() const { return D_ * D_ * D_ * D_; }
  size_t size() const { return rows_ * cols_; }
  TenElemT *component(size_t r, size_t c, size_t s) { return v_.data() + ((r * cols_ + c) * d_ + s) * slot(); }
  const TenElemT *component(size_t r, size_t c, size_t s) const { return v_.data() + ((r * cols_ + c) * d_ + s) * slot(); }
  std::vector<TenElemT> &flat() { return v_; }
  const std::vector<TenElemT> &flat() const { return v_; }
  double NormSquare() const { double a = 0.0; for (const auto &x : v_) a += AbsSquare(x); return a; }

  // SplitIndexTPS::Load (split_index_tps_impl.h:340-437): tps_meta.txt + tps_ten{r}_{c}_{s}.qlten,
  // dense TrivialRepQN payloads only: float64, or interleaved complex128 for QLTEN_Complex (format: SURVEY.md section 8c).
  static SplitIndexTPST Load(const std::string &dir, size_t D) {
    std::ifstream meta(dir + "/tps_meta.txt");
    if (!meta) throw std::runtime_error("SplitIndexTPS::Load: cannot open " + dir + "/tps_meta.txt");
    long rows_l = 0, cols_l = 0, d_l = 0, bc = 0;
    if (!(meta >> rows_l >> cols_l >> d_l) || rows_l <= 0 || cols_l <= 0 || d_l <= 0 || rows_l > 4096 || cols_l > 4096 || d_l > 4096)
      throw std::runtime_error("SplitIndexTPS::Load: malformed tps_meta.txt (rows cols phy_dim [bc]) in " + dir);
    // 4th field = BoundaryCondition (split_index_tps_impl.h:346-353; absent in old files = Open).  The device path is
    // OBC only: a periodic state must not load silently as an open one.
    if ((meta >> bc) && bc != 0)
      throw std::runtime_error("SplitIndexTPS::Load: boundary condition " + std::to_string(bc) + " (not Open) is not supported");
    const size_t rows = (size_t)rows_l, cols = (size_t)cols_l, d = (size_t)d_l;
    SplitIndexTPST t(rows, cols, d, D);
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < cols; ++c)
        for (size_t s = 0; s < d; ++s) {
          std::string path = dir + "/tps_ten" + std::to_string(r) + "_" + std::to_string(c) + "_" + std::to_string(s) + ".qlten";
          std::ifstream f(path, std::ios::binary);
          if (!f) throw std::runtime_error("SplitIndexTPS::Load: cannot open " + path);
          std::string line;
          auto next = [&]() {
            if (!std::getline(f, line)) throw std::runtime_error("SplitIndexTPS::Load: truncated header in " + path);
            try { return std::stoll(line); } catch (const std::exception &) {
              throw std::runtime_error("SplitIndexTPS::Load: malformed header in " + path);
            }
          };
          long rank = next();
          if (rank != 4) throw std::runtime_error("SplitIndexTPS::Load: rank-4 dense tensors only");
          size_t dims[4];
          for (int k = 0; k < 4; ++k) {
            long nsec = next();
            if (nsec != 1) throw std::runtime_error("SplitIndexTPS::Load: block-sparse tensors are not supported");
            next(); next();          // degeneracy, sector hash
            next();                  // direction
            dims[k] = (size_t)next();
            std::getline(f, line);   // index hash (u64, may exceed long)
          }
          long nblocks = next();
          if (nblocks != 1) throw std::runtime_error("SplitIndexTPS::Load: expected one dense block");
          for (int k = 0; k < 4; ++k) next();
          for (int k = 0; k < 4; ++k)
            if (dims[k] == 0 || dims[k] > D)
              throw std::runtime_error("SplitIndexTPS::Load: leg " + std::to_string(k) + " of " + path + " has dimension " +
                                       std::to_string(dims[k]) + ", the caller's bond dimension is " + std::to_string(D));
          std::vector<TenElemT> buf(dims[0] * dims[1] * dims[2] * dims[3]);
          f.read(reinterpret_cast<char *>(buf.data()), buf.size() * sizeof(TenElemT));
          if (!f) throw std::runtime_error("SplitIndexTPS::Load: truncated payload in " + path);
          TenElemT *dst = t.component(r, c, s);
          size_t o = 0;
          for (size_t a = 0; a < dims[0]; ++a)
            for (size_t b = 0; b < dims[1]; ++b)
              for (size_t cc = 0; cc < dims[2]; ++cc)
                for (size_t e = 0; e < dims[3]; ++e) dst[((a * D + b) * D + cc) * D + e] = buf[o++];
        }
    return t;
  }

  // SplitIndexTPS::Dump (split_index_tps_impl.h:300-330): the same files Load reads, byte-identical
  // to the reference's for dense TrivialRepQN tensors (round trip of the reference fixtures is the
  // test).  dims(r, c) = the true (un-padded) leg dimensions (L, D, R, U); OBC default: boundary legs 1.
  static uint64_t TrivialIndexHash(int dir, uint64_t dim) {
    // index_hash = VecHash({sector_hash}) ^ std::hash<int>(dir), sector_hash = 0 ^ degeneracy; VecHash is the
    // xxHash-style tuple hash (recovered from the 168 fixture files of the reference, 8 distinct (dir, dim) pairs)
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P5 = 0x27D4EB2F165667C5ull;
    uint64_t acc = P5 + dim * P2;
    acc = (acc << 31) | (acc >> 33);
    acc *= P1;
    acc += (1ull ^ P5);
    return acc ^ (dir == 1 ? 1ull : ~0ull);
  }
  void Dump(const std::string &dir, const std::function<std::array<size_t, 4>(size_t, size_t)> &dims = nullptr) const {
    auto obc = [&](size_t r, size_t c) {
      return std::array<size_t, 4>{c == 0 ? 1 : D_, r + 1 == rows_ ? 1 : D_, c + 1 == cols_ ? 1 : D_, r == 0 ? 1 : D_};
    };
    const int dirs[4] = {-1, 1, 1, -1};   // (L, D, R, U) = IN, OUT, OUT, IN in every reference fixture
    for (size_t r = 0; r < rows_; ++r)
      for (size_t c = 0; c < cols_; ++c) {
        const std::array<size_t, 4> dd = dims ? dims(r, c) : obc(r, c);
        for (size_t s = 0; s < d_; ++s) {
          std::string path = dir + "/tps_ten" + std::to_string(r) + "_" + std::to_string(c) + "_" + std::to_string(s) + ".qlten";
          std::ofstream f(path, std::ios::binary);
          if (!f) throw std::ios_base::failure("Failed to open file: " + path);
          f << 4 << "\n";
          for (int k = 0; k < 4; ++k)
            f << 1 << "\n" << dd[k] << "\n" << dd[k] << "\n" << dirs[k] << "\n" << dd[k] << "\n" << TrivialIndexHash(dirs[k], dd[k]) << "\n";
          f << 1 << "\n0\n0\n0\n0\n";
          const TenElemT *src = component(r, c, s);
          std::vector<TenElemT> buf;
          buf.reserve(dd[0] * dd[1] * dd[2] * dd[3]);
          for (size_t a = 0; a < dd[0]; ++a)
            for (size_t b = 0; b < dd[1]; ++b)
              for (size_t cc = 0; cc < dd[2]; ++cc)
                for (size_t e = 0; e < dd[3]; ++e) buf.push_back(src[((a * D_ + b) * D_ + cc) * D_ + e]);
          f.write(reinterpret_cast<const char *>(buf.data()), buf.size() * sizeof(TenElemT));
          f << "\n";
          if (!f) throw std::ios_base::failure("Failed to write: " + path);
        }
      }
    std::ofstream meta(dir + "/tps_meta.txt", std::ios::binary);
    if (!meta) throw std::ios_base::failure("Failed to open metadata file: " + dir + "/tps_meta.txt");
    meta << rows_ << " " << cols_ << " " << d_ << " " << 0;   // BoundaryCondition::Open
  }

 private:
  size_t rows_ = 0, cols_ = 0, d_ = 0, D_ = 0;
  std::vector<TenElemT> v_;
};
using SplitIndexTPS = SplitIndexTPST<double>;

// Configuration::Dump / Load for one walker (configuration.h:270-393): text matrix `configuration{label}` + the `.shape` sidecar.
// Dump creates the directory (EnsureDirectoryExists) and throws std::ios_base::failure when the file cannot be written; Load never throws:
// it returns false for a missing file, a sidecar whose (rows, cols) differ from the object's, or a payload that does not parse
// (:356-393).  StreamReadConfiguration is Configuration::StreamRead (:420-440): throws std::runtime_error on short input.
inline void EnsureDirectoryExists(const std::string &d) {
  for (size_t k = 1; k <= d.size(); ++k)
    if (k == d.size() || d[k] == '/') ::mkdir(d.substr(0, k).c_str(), 0755);
}
inline void StreamReadConfiguration(Configuration &cfg, size_t walker, std::istream &is) {
  for (size_t r = 0; r < cfg.rows(); ++r)
    for (size_t c = 0; c < cfg.cols(); ++c)
      if (!(is >> cfg(walker, {r, c})))
        throw std::runtime_error("Configuration::StreamRead: Failed to read data from stream (row " + std::to_string(r) +
                                 ", col " + std::to_string(c) + ")");
}
inline void DumpConfiguration(const Configuration &cfg, size_t walker, const std::string &directory, size_t label) {
  EnsureDirectoryExists(directory);
  const std::string file = directory + "/configuration" + std::to_string(label);
  std::ofstream ofs(file, std::ofstream::binary);
  if (!ofs.is_open()) throw std::ios_base::failure("Failed to open file: " + file);
  for (size_t r = 0; r < cfg.rows(); ++r) {
    for (size_t c = 0; c + 1 < cfg.cols(); ++c) ofs << cfg(walker, {r, c}) << " ";
    ofs << cfg(walker, {r, cfg.cols() - 1}) << std::endl;
  }
  if (ofs.fail()) throw std::ios_base::failure("Failed to write configuration to file: " + file);
  std::ofstream sofs(file + ".shape");
  if (sofs.is_open()) sofs << cfg.rows() << " " << cfg.cols() << "\n";
}
inline bool LoadConfiguration(Configuration &cfg, size_t walker, const std::string &directory, size_t label) {
  const std::string file = directory + "/configuration" + std::to_string(label);
  {
    std::ifstream sifs(file + ".shape");                     // (files of older versions have no sidecar)
    if (sifs.is_open()) {
      size_t rows = 0, cols = 0;
      if (!(sifs >> rows >> cols)) return false;
      if (rows != cfg.rows() || cols != cfg.cols()) return false;
    }
  }
  std::ifstream ifs(file, std::ifstream::binary);
  if (!ifs.is_open()) return false;
  try {
    StreamReadConfiguration(cfg, walker, ifs);
  } catch (...) {
    return false;
  }
  return !ifs.fail();
}

// BMPSContractor (bmps_contractor.h:187-1027): same method names; `tn` arguments disappear because
// the projected network is (sitps, configs) held by the context.  Scalars come back per walker.
template <typename TenElemT>
class BMPSContractorT {
 public:
  BMPSContractorT(size_t rows, size_t cols, size_t D, size_t phys_dim, const BMPSTruncateParams &p, size_t max_walkers,
                 int dtype = PEPSGPU_F64, int device = 0)
      : rows_(rows), cols_(cols), D_(D), d_(phys_dim), trunc_(p) {
    int rc = pepsgpu_ctx_create(&ctx_, device, ElemTraits<TenElemT>::ctx_dtype(dtype), (int)rows, (int)cols, (int)D, (int)phys_dim, (int)p.D_min,
                                (int)p.D_max, p.trunc_err, (int)p.compress_scheme, (int)max_walkers);
    if (rc != PEPSGPU_OK) { ctx_ = nullptr; check_rc(rc, nullptr); }
    if (p.compress_scheme != CompressMPSScheme::SVD_COMPRESS) SetTruncateParams(p);
  }
  ~BMPSContractorT() { if (ctx_) pepsgpu_ctx_destroy(ctx_); }
  // bmps_contractor.h:216; the variational schemes need convergence_tol and iter_max (bmps_impl.h:425-430 .value())
  void SetTruncateParams(const BMPSTruncateParams &p) {
    if (p.compress_scheme != CompressMPSScheme::SVD_COMPRESS && !(p.convergence_tol && p.iter_max))
      throw std::invalid_argument("variational compression needs convergence_tol and iter_max");
    check_rc(pepsgpu_set_truncate_params(ctx_, (int)p.D_min, (int)p.D_max, p.trunc_err, (int)p.compress_scheme,
                                         p.convergence_tol.value_or(0.0), (int)p.iter_max.value_or(0)), ctx_);
    trunc_ = p;
  }
  BMPSContractorT(const BMPSContractorT &) = delete;
  BMPSContractorT &operator=(const BMPSContractorT &) = delete;

  pepsgpu_ctx *ctx() const { return ctx_; }
  size_t rows() const { return rows_; }
  size_t cols() const { return cols_; }
  size_t walkers() const { return (size_t)pepsgpu_n_walkers(ctx_); }
  size_t phys_dim() const { return d_; }                  // states per site on the device (fermions: the 4 d extended states)
  size_t bond_dim() const { return D_; }
  const BMPSTruncateParams &GetTruncateParams() const { return trunc_; }

  void UploadState(const SplitIndexTPST<TenElemT> &s) { check_rc(pepsgpu_state_upload(ctx_, dptr(s.flat().data()), ElemTraits<TenElemT>::host_dtype), ctx_); }
  void Init(const Configuration &cfg) { check_rc(pepsgpu_walkers_set_configs(ctx_, (int)cfg.walkers(), cfg.data()), ctx_); }

  void GrowBMPSStep(BMPSPOSITION p) { check_rc(pepsgpu_grow_bmps_step(ctx_, p), ctx_); }
  void GrowFullBMPS(BMPSPOSITION p) { check_rc(pepsgpu_grow_full_bmps(ctx_, p), ctx_); }
  void GrowBMPSForRow(size_t row) { check_rc(pepsgpu_grow_bmps_for_row(ctx_, (int)row), ctx_); }
  void GrowBMPSForCol(size_t col) { check_rc(pepsgpu_grow_bmps_for_col(ctx_, (int)col), ctx_); }
  void ShiftBMPSWindow(BMPSPOSITION p) { check_rc(pepsgpu_shift_bmps_window(ctx_, p), ctx_); }
  void DeleteInnerBMPS(BMPSPOSITION p) { check_rc(pepsgpu_delete_inner_bmps(ctx_, p), ctx_); }
  // BMPSWalker equivalents (bmps_walker.h): the stack is the walker, the opposite environment is named by parking
  void ParkBMPS(BMPSPOSITION p, size_t keep_levels) { check_rc(pepsgpu_bmps_park(ctx_, p, (int)keep_levels), ctx_); }
  void UnparkBMPS(BMPSPOSITION p) { check_rc(pepsgpu_bmps_unpark(ctx_, p), ctx_); }
  void GenerateBMPSApproach(BMPSPOSITION p) { check_rc(pepsgpu_generate_bmps_approach(ctx_, p), ctx_); }

  // BMPSContractor::BMPSWalker (bmps_contractor.h:357-646, bmps/impl/bmps_walker.h): the object form.  One C++ walker holds the
  // fork for every Monte-Carlo walker of the context; where the reference passes `const TransferMPO &mpo` and
  // `const BMPS &opposite_boundary` to every call, the MPO is named once (SetMPO*: a row of the network under the walkers'
  // configurations, under per-walker states, or explicit tensors -- an MPO that is not a row of the network) and the opposite
  // boundary is the level of the DOWN stack (`down_stack[opp_level]` in the reference's tests).  Same method names, same
  // std::runtime_error conditions (size / direction / cache checks of bmps_walker.h).
  class BMPSWalker {
   public:
    BMPSWalker(BMPSWalker &&o) noexcept : ctx_(o.ctx_), id_(o.id_), n_(o.n_), cols_(o.cols_) { o.id_ = -1; }
    BMPSWalker(const BMPSWalker &) = delete;
    BMPSWalker &operator=(const BMPSWalker &) = delete;
    ~BMPSWalker() { if (id_ >= 0) (void)pepsgpu_walker_destroy(ctx_, id_); }
    void EvolveStep() { check_rc(pepsgpu_walker_evolve_step(ctx_, id_), ctx_); }
    void SetMPO(size_t num) { check_rc(pepsgpu_walker_set_mpo(ctx_, id_, (int)num, nullptr, nullptr, 0), ctx_); }
    // states[w][j]: component of site j of slice `num` for Monte-Carlo walker w
    void SetMPOStates(size_t num, const std::vector<int32_t> &states) { check_rc(pepsgpu_walker_set_mpo(ctx_, id_, (int)num, states.data(), nullptr, 0), ctx_); }
    // tensors[q][j][D^4] (leg order L, D, R, U, zero padded to D), n_tensors = 1 (shared) or the number of walkers
    void SetMPOTensors(size_t num, const std::vector<TenElemT> &tensors, size_t n_tensors) {
      check_rc(pepsgpu_walker_set_mpo(ctx_, id_, (int)num, nullptr, dptr(tensors.data()), (int)n_tensors), ctx_);
    }
    // The excited row of the structure-factor mixin (structure_factor_measurement_mixin.h:127-134) built on the device: row `num`
    // under the walkers' configurations with the state s of site `col` replaced by state_map[s]; returns open[w] = the map
    // changes walker w's state.  Same walker afterwards as SetMPOStates with that row.
    std::vector<uint8_t> SetMPOExcited(size_t num, size_t col, const std::vector<int32_t> &state_map) {
      std::vector<uint8_t> open(n_);
      check_rc(pepsgpu_walker_set_mpo_excited(ctx_, id_, (int)num, (int)col, state_map.data(), open.data()), ctx_);
      return open;
    }
    // The scan of one target row (:160-194) in one call: InitBTenLeft(opp, Lx), InitBTenRight(opp, Lx - 1), then right to left
    // TraceWithBTen with the site's state s replaced by site_map[s] + GrowBTenRightStep.  [w][x2]: the trace where mask[w] (empty:
    // every walker) and site_map[s] != s, exactly 0 elsewhere.
    std::vector<TenElemT> TraceSlice(size_t opp_level, const std::vector<int32_t> &site_map, const std::vector<uint8_t> &mask = {}) {
      std::vector<TenElemT> out(n_ * cols_);
      check_rc(pepsgpu_walker_trace_slice(ctx_, id_, (int)opp_level, site_map.data(), mask.empty() ? nullptr : mask.data(), dptr(out.data())),
               ctx_);
      return out;
    }
    // The excited row of the singlet-pair correlation (singlet_pair_correlation_measurement_mixin.h:376-401) built on the device: row
    // `num` of a fermionic context with the pair (col, col + 1) replaced by candidate `slot` of pair_table ([d * d][2][2] over
    // physical states, occ [d] their fermion numbers).  Returns open[w] = the walker has the candidate; sign (optional) receives
    // Sigma(S') / Sigma(S) per walker, 0 for none.  Same walker afterwards as SetMPOStates with that row.
    std::vector<uint8_t> SetMPOExcitedPair(size_t num, size_t col, const std::vector<int32_t> &occ, const std::vector<int32_t> &pair_table,
                                           int slot, std::vector<int32_t> *sign = nullptr) {
      std::vector<uint8_t> open(n_);
      std::vector<int32_t> sg(n_);
      check_rc(pepsgpu_walker_set_mpo_excited_pair(ctx_, id_, (int)num, (int)col, (int)occ.size(), occ.data(), pair_table.data(), slot,
                                                   open.data(), sg.data()), ctx_);
      if (sign) sign->swap(sg);
      return open;
    }
    // The scan of one target row (:446-519) in one call: InitBTenLeft(opp, 0), InitBTenRight(opp, 1), then left to right
    // TraceWithTwoSiteBTen with the pair's states replaced by candidate k of pair_table + ShiftBTenWindow(RIGHT).  [w][x2][k]: sign *
    // trace where mask[w] (empty: every walker) and the candidate exists, exactly 0 elsewhere.
    std::vector<TenElemT> PairTraceSlice(size_t opp_level, const std::vector<int32_t> &occ, const std::vector<int32_t> &pair_table,
                                         const std::vector<uint8_t> &mask = {}) {
      std::vector<TenElemT> out(n_ * (cols_ - 1) * 2);
      check_rc(pepsgpu_walker_pair_trace_slice(ctx_, id_, (int)opp_level, (int)occ.size(), occ.data(), pair_table.data(),
                                               mask.empty() ? nullptr : mask.data(), dptr(out.data())), ctx_);
      return out;
    }
    void Evolve() { check_rc(pepsgpu_walker_evolve(ctx_, id_), ctx_); }
    std::vector<TenElemT> ContractRow(size_t opp_level) const {
      std::vector<TenElemT> out(n_);
      check_rc(pepsgpu_walker_contract_row(ctx_, id_, (int)opp_level, dptr(out.data())), ctx_);
      return out;
    }
    void InitBTenLeft(size_t opp_level, size_t target_col) { check_rc(pepsgpu_walker_init_bten(ctx_, id_, (int)opp_level, LEFT, (int)target_col), ctx_); }
    void InitBTenRight(size_t opp_level, size_t target_col) { check_rc(pepsgpu_walker_init_bten(ctx_, id_, (int)opp_level, RIGHT, (int)target_col), ctx_); }
    void GrowBTenLeftStep(size_t opp_level) { check_rc(pepsgpu_walker_grow_bten_step(ctx_, id_, (int)opp_level, LEFT), ctx_); }
    void GrowBTenRightStep(size_t opp_level) { check_rc(pepsgpu_walker_grow_bten_step(ctx_, id_, (int)opp_level, RIGHT), ctx_); }
    void ShiftBTenWindow(size_t opp_level, BTenPOSITION position) { check_rc(pepsgpu_walker_shift_bten_window(ctx_, id_, (int)opp_level, position), ctx_); }
    // replacement site(s): SITPS component per walker (states[w], or states[w][2] for the two-site form); empty = the MPO's own
    std::vector<TenElemT> TraceWithBTen(size_t opp_level, size_t site_col, const std::vector<int32_t> &states = {}) const {
      std::vector<TenElemT> out(n_);
      check_rc(pepsgpu_walker_trace_with_bten(ctx_, id_, (int)opp_level, (int)site_col, 0, states.empty() ? nullptr : states.data(), nullptr, 0,
                                              dptr(out.data())), ctx_);
      return out;
    }
    std::vector<TenElemT> TraceWithBTenTensor(size_t opp_level, size_t site_col, const std::vector<TenElemT> &site, size_t n_tensors) const {
      std::vector<TenElemT> out(n_);
      check_rc(pepsgpu_walker_trace_with_bten(ctx_, id_, (int)opp_level, (int)site_col, 0, nullptr, dptr(site.data()), (int)n_tensors,
                                              dptr(out.data())), ctx_);
      return out;
    }
    std::vector<TenElemT> TraceWithTwoSiteBTen(size_t opp_level, size_t site_col, const std::vector<int32_t> &states_ab = {}) const {
      std::vector<TenElemT> out(n_);
      check_rc(pepsgpu_walker_trace_with_bten(ctx_, id_, (int)opp_level, (int)site_col, 1, states_ab.empty() ? nullptr : states_ab.data(), nullptr,
                                              0, dptr(out.data())), ctx_);
      return out;
    }
    void ClearBTen() { check_rc(pepsgpu_walker_clear_bten(ctx_, id_), ctx_); }
    BMPSWalker Clone() const {                      // `auto excited_walker = main_walker;`
      int id = -1;
      check_rc(pepsgpu_walker_clone(ctx_, id_, &id), ctx_);
      return BMPSWalker(ctx_, id, n_, cols_);
    }
    size_t GetBTenLeftCol() const { return (size_t)info(2); }
    size_t GetBTenRightCol() const { return (size_t)info(3); }
    size_t GetStackSize() const { return (size_t)info(1); }
    BMPSPOSITION GetPosition() const { return (BMPSPOSITION)info(0); }

   private:
    friend class BMPSContractorT;
    BMPSWalker(pepsgpu_ctx *ctx, int id, size_t n, size_t cols) : ctx_(ctx), id_(id), n_(n), cols_(cols) {}
    int info(int k) const {
      int v[4];
      check_rc(pepsgpu_walker_info(ctx_, id_, &v[0], &v[1], &v[2], &v[3]), ctx_);
      return v[k];
    }
    pepsgpu_ctx *ctx_;
    int id_;
    size_t n_, cols_;
  };
  // GetWalker(tn, position) (bmps_walker.h:51-58): a detached copy of the top of the stack
  BMPSWalker GetWalker(BMPSPOSITION position) const {
    int id = -1;
    check_rc(pepsgpu_walker_create(ctx_, position, -1, &id), ctx_);
    return BMPSWalker(ctx_, id, walkers(), cols_);
  }
  // BMPSWalker(tn, GetBMPS(position)[level], position, level + 1, trunc_params): the constructor the structure-factor mixin
  // uses on the vacuum (structure_factor_measurement_mixin.h:121-122)
  BMPSWalker MakeWalker(BMPSPOSITION position, size_t level) const {
    int id = -1;
    check_rc(pepsgpu_walker_create(ctx_, position, (int)level, &id), ctx_);
    return BMPSWalker(ctx_, id, walkers(), cols_);
  }

  void InitBTen(BTenPOSITION p, size_t slice) { check_rc(pepsgpu_init_bten(ctx_, p, (int)slice), ctx_); }
  void GrowFullBTen(BTenPOSITION p, size_t slice, size_t remain_sites = 2, bool init = true) {
    check_rc(pepsgpu_grow_full_bten(ctx_, p, (int)slice, (int)remain_sites, init), ctx_);
  }
  void GrowBTenStep(BTenPOSITION p) { check_rc(pepsgpu_grow_bten_step(ctx_, p), ctx_); }
  void ShiftBTenWindow(BTenPOSITION p) { check_rc(pepsgpu_shift_bten_window(ctx_, p), ctx_); }
  void TruncateBTen(BTenPOSITION p, size_t len) { check_rc(pepsgpu_truncate_bten(ctx_, p, (int)len), ctx_); }
  void EraseEnvsAfterUpdate(const SiteIdx &s) { check_rc(pepsgpu_erase_envs_after_update(ctx_, (int)s.r, (int)s.c), ctx_); }
  // CheckInvalidateEnvs (trace.h:591-626): no cached environment may cross `site` after an accepted
  // move.  The reference asserts in debug builds; here the check always runs and throws.
  void CheckInvalidateEnvs(const SiteIdx &s) const {
    const int lim[4] = {(int)s.c + 1, (int)(rows_ - s.r), (int)(cols_ - s.c), (int)s.r + 1};   // LEFT, DOWN, RIGHT, UP
    for (int pos = 0; pos < 4; ++pos)
      if (pepsgpu_bmps_stack_size(ctx_, pos) > lim[pos] || pepsgpu_bten_stack_size(ctx_, pos) > lim[pos] ||
          pepsgpu_bten2_stack_size(ctx_, pos) > lim[pos])
        throw std::logic_error("BMPSContractor::CheckInvalidateEnvs: stale environment beyond the updated site");
  }
  // DirectionCheck (grow.h:185-198): a stack only ever holds BMPS of its own direction here (the
  // direction is the stack index on the device), so the invariant holds by construction.
  bool DirectionCheck() const { return true; }
  size_t BMPSStackSize(BMPSPOSITION p) const { return (size_t)pepsgpu_bmps_stack_size(ctx_, p); }   // GetBMPS(p).size()
  // Host copy of one boundary MPS, GetBMPS(pos)[level] (bmps_contractor.h:236-247): tensors[i] is
  // [walker][d0*d1*d2] with dims[i], times exp(logscale[walker]).  The gauge differs from the reference.
  struct BMPSHost {
    std::vector<std::array<int, 3>> dims;
    std::vector<std::vector<TenElemT>> tensors;
    std::vector<double> logscale;
  };
  BMPSHost GetBMPS(BMPSPOSITION p, size_t level) const {
    const size_t len = (p == UP || p == DOWN) ? cols_ : rows_, n = walkers();
    BMPSHost b;
    b.dims.resize(len); b.tensors.resize(len); b.logscale.assign(n, 0.0);
    for (size_t i = 0; i < len; ++i) {
      int d[3];
      check_rc(pepsgpu_get_bmps_tensor(ctx_, p, (int)level, (int)i, d, nullptr, nullptr), ctx_);
      b.dims[i] = {d[0], d[1], d[2]};
      b.tensors[i].resize(n * (size_t)d[0] * d[1] * d[2]);
      check_rc(pepsgpu_get_bmps_tensor(ctx_, p, (int)level, (int)i, d, dptr(b.tensors[i].data()), b.logscale.data()), ctx_);
    }
    return b;
  }
  // GetBMPSForRow / GetBMPSForCol (grow.h:124-141): grow, then the (UP, DOWN) / (LEFT, RIGHT) pair of the slice
  std::pair<BMPSHost, BMPSHost> GetBMPSForRow(size_t row) {
    GrowBMPSForRow(row);
    return {GetBMPS(UP, row), GetBMPS(DOWN, rows_ - 1 - row)};
  }
  std::pair<BMPSHost, BMPSHost> GetBMPSForCol(size_t col) {
    GrowBMPSForCol(col);
    return {GetBMPS(LEFT, col), GetBMPS(RIGHT, cols_ - 1 - col)};
  }

  std::vector<TenElemT> Trace(const SiteIdx &a, BondOrientation dir) const {
    std::vector<TenElemT> out(walkers());
    check_rc(pepsgpu_trace(ctx_, (int)a.r, (int)a.c, dir, dptr(out.data())), ctx_);
    return out;
  }
  // ReplaceNNSiteTrace for n_cand candidate (state_a, state_b) pairs per walker: cand[w][k][2]
  std::vector<TenElemT> ReplaceNNSiteTrace(const SiteIdx &a, BondOrientation dir, int n_cand, const std::vector<int32_t> &cand) const {
    std::vector<TenElemT> out(walkers() * n_cand);
    check_rc(pepsgpu_replace_nn_trace(ctx_, (int)a.r, (int)a.c, dir, n_cand, cand.data(), dptr(out.data())), ctx_);
    return out;
  }
  std::vector<TenElemT> ReplaceOneSiteTrace(const SiteIdx &s, BondOrientation orient, int n_cand, const std::vector<int32_t> &cand) const {
    std::vector<TenElemT> out(walkers() * n_cand);
    check_rc(pepsgpu_replace_one_trace(ctx_, (int)s.r, (int)s.c, orient, n_cand, cand.data(), dptr(out.data())), ctx_);
    return out;
  }
  // Two-row environments (bten_set2_): init.h:130-186, grow.h:375-527
  void InitBTen2(BTenPOSITION p, size_t slice_num1) { check_rc(pepsgpu_init_bten2(ctx_, p, (int)slice_num1), ctx_); }
  void GrowFullBTen2(BTenPOSITION p, size_t slice_num1, size_t remain_sites = 2, bool init = true) {
    check_rc(pepsgpu_grow_full_bten2(ctx_, p, (int)slice_num1, (int)remain_sites, init), ctx_);
  }
  void GrowBTen2Step(BTenPOSITION p, size_t slice_num1) { check_rc(pepsgpu_grow_bten2_step(ctx_, p, (int)slice_num1), ctx_); }
  void ShiftBTen2Window(BTenPOSITION p, size_t slice_num1) { check_rc(pepsgpu_shift_bten2_window(ctx_, p, (int)slice_num1), ctx_); }
  // trace.h:207-324 / :326-423 / :425-536; cand[w][k][2|3|2], n_cand = 0: no replacement
  std::vector<TenElemT> ReplaceNNNSiteTrace(const SiteIdx &left_up, DIAGONAL_DIR nnn_dir, BondOrientation orient, int n_cand,
                                          const std::vector<int32_t> &cand) const {
    std::vector<TenElemT> out(walkers() * (n_cand > 0 ? n_cand : 1));
    check_rc(pepsgpu_replace_nnn_trace(ctx_, (int)left_up.r, (int)left_up.c, nnn_dir, orient, n_cand,
                                       n_cand > 0 ? cand.data() : nullptr, dptr(out.data())), ctx_);
    return out;
  }
  // Second BTen2 set, one-slice configuration override and the four-tensor plaquette trace: the environment-reusing diagonal hop
  // of a fermionic state (SquareSpinlessFermion::AddNNNHopEnergyLocal below; include/pepsgpu.h has the statement)
  void SelectBTen2Set(int set) { check_rc(pepsgpu_bten2_select_set(ctx_, set), ctx_); }
  void OverrideSlice(BondOrientation orient, size_t num, const std::vector<int32_t> *states) {
    // (the C ABI carries no length: the engine reads states[w * N + j], N = columns of a row / rows of a column)
    if (states && states->size() != walkers() * (orient == HORIZONTAL ? cols() : rows()))
      throw std::invalid_argument("OverrideSlice: states must hold walkers x (length of the slice) entries");
    check_rc(pepsgpu_cfg_override_slice(ctx_, orient, (int)num, states ? states->data() : nullptr), ctx_);
  }
  std::vector<TenElemT> ReplacePlaquetteTrace(const SiteIdx &left_up, int n_cand, const std::vector<int32_t> &cand, int left_set,
                                            int right_set) const {
    std::vector<TenElemT> out(walkers() * (n_cand > 0 ? n_cand : 1));
    check_rc(pepsgpu_replace_plaquette_trace(ctx_, (int)left_up.r, (int)left_up.c, n_cand, n_cand > 0 ? cand.data() : nullptr, left_set,
                                             right_set, dptr(out.data())), ctx_);
    return out;
  }
  std::vector<TenElemT> ReplaceTNNSiteTrace(const SiteIdx &site0, BondOrientation orient, int n_cand,
                                          const std::vector<int32_t> &cand) const {
    std::vector<TenElemT> out(walkers() * (n_cand > 0 ? n_cand : 1));
    check_rc(pepsgpu_replace_tnn_trace(ctx_, (int)site0.r, (int)site0.c, orient, n_cand,
                                       n_cand > 0 ? cand.data() : nullptr, dptr(out.data())), ctx_);
    return out;
  }
  std::vector<TenElemT> ReplaceSqrt5DistTwoSiteTrace(const SiteIdx &left_up, DIAGONAL_DIR link_dir, BondOrientation orient,
                                                   int n_cand, const std::vector<int32_t> &cand) const {
    std::vector<TenElemT> out(walkers() * (n_cand > 0 ? n_cand : 1));
    check_rc(pepsgpu_replace_sqrt5_trace(ctx_, (int)left_up.r, (int)left_up.c, link_dir, orient, n_cand,
                                         n_cand > 0 ? cand.data() : nullptr, dptr(out.data())), ctx_);
    return out;
  }
  // PunchHole: [walker][D^4] (legs L,D,R,U zero padded)
  std::vector<TenElemT> PunchHole(const SiteIdx &s, BondOrientation orient) const {
    std::vector<TenElemT> out(walkers() * D_ * D_ * D_ * D_);
    check_rc(pepsgpu_punch_hole(ctx_, (int)s.r, (int)s.c, orient, dptr(out.data())), ctx_);
    return out;
  }
  // Device-resident variant: the hole stays in HBM for GradAccumulate (no PCIe round trip)
  void PunchHoleStore(const SiteIdx &s, BondOrientation orient) {
    check_rc(pepsgpu_punch_hole(ctx_, (int)s.r, (int)s.c, orient, nullptr), ctx_);
  }
  void GradReset() { check_rc(pepsgpu_grad_reset(ctx_), ctx_); }
  void GradAccumulate(const std::vector<TenElemT> &psi, const std::vector<TenElemT> &eloc, bool exact_sum) {
    check_rc(pepsgpu_grad_accumulate(ctx_, dptr(psi.data()), dptr(eloc.data()), exact_sum), ctx_);
  }
  // ... with the component of every site named by the caller ([walker][row][col]): fermionic states
  void GradAccumulate(const std::vector<TenElemT> &psi, const std::vector<TenElemT> &eloc, bool exact_sum,
                      const std::vector<int32_t> &states) {
    if (states.size() != walkers() * rows() * cols()) throw std::invalid_argument("GradAccumulate: states must be [walker][row][col]");
    check_rc(pepsgpu_grad_accumulate_states(ctx_, dptr(psi.data()), dptr(eloc.data()), exact_sum, states.data()), ctx_);
  }
  // ---- the exchange step over ranks (one contractor = one GPU = one rank): RCCL through the library ----
  // CommInit: rank 0 draws `id` with UniqueId() and the host program broadcasts it (MPI_Bcast in the reference's MPI world).
  static std::array<unsigned char, 128> UniqueId() {
    std::array<unsigned char, 128> id{};
    check_rc(pepsgpu_comm_unique_id(id.data()), nullptr);
    return id;
  }
  void CommInit(int nranks, int rank, const std::array<unsigned char, 128> *id) {
    check_rc(pepsgpu_comm_init(ctx_, nranks, rank, id ? id->data() : nullptr), ctx_);
  }
  int CommSize() const { return pepsgpu_comm_size(ctx_); }
  int CommRank() const { return pepsgpu_comm_rank(ctx_); }
  // S_O, S_EO summed over the ranks in HBM (replaces MPIMeanTensor, statistics_tensor.h:37-79)
  void GradAllReduce() { check_rc(pepsgpu_grad_allreduce(ctx_), ctx_); }
  // small host vectors (energies, weights, acceptance rates): staged through HBM, same communicator
  void AllReduceSum(std::vector<double> &v) { check_rc(pepsgpu_allreduce(ctx_, v.data(), (long)v.size(), 1, 0, 0), ctx_); }
  void AllReduceMax(std::vector<double> &v) { check_rc(pepsgpu_allreduce(ctx_, v.data(), (long)v.size(), 1, 1, 0), ctx_); }
  // the reducer the evaluators take (std::function<void(std::vector<double>&)>), bound to this contractor's communicator
  std::function<void(std::vector<double> &)> RcclReducer() {
    return [this](std::vector<double> &v) { AllReduceSum(v); };
  }
  void GradRead(std::vector<TenElemT> &so, std::vector<TenElemT> &seo) const {
    const size_t n = rows_ * cols_ * d_ * D_ * D_ * D_ * D_;
    so.resize(n); seo.resize(n);
    check_rc(pepsgpu_grad_read(ctx_, dptr(so.data()), dptr(seo.data())), ctx_);
  }
  // device-resident optimisation step (pepsgpu_opt_*): theta, the gradient / direction and the rule state stay in HBM
  // d stored states with parities nf, bond parities [rows][cols][4][D]: the optimizer calls below then keep their vectors in the
  // range of the decoration and report norms over the stored parameters; d = 0 clears it
  void FermionDecorationSet(const std::vector<int> &nf, const std::vector<uint8_t> &bond_parity) {
    std::vector<int32_t> n32(nf.begin(), nf.end());
    check_rc(pepsgpu_fermion_decoration_set(ctx_, (int)n32.size(), n32.data(), bond_parity.data()), ctx_);
  }
  void FermionDecorationClear() { check_rc(pepsgpu_fermion_decoration_set(ctx_, 0, nullptr, nullptr), ctx_); }
  void OptBegin() { check_rc(pepsgpu_opt_begin(ctx_), ctx_); }
  void OptEnd() { check_rc(pepsgpu_opt_end(ctx_), ctx_); }
  // g <- (S_EO - conj(E) S_O) / W from the resident accumulators; returns (E, |g|)
  std::pair<TenElemT, double> OptGradientFromAccumulators(const TenElemT &e_loc_sum, double weight_sum) {
    TenElemT e(0.0);
    double nrm = 0.0;
    check_rc(pepsgpu_opt_gradient_from_accumulators(ctx_, dptr(&e_loc_sum), weight_sum, dptr(&e), &nrm), ctx_);
    return {e, nrm};
  }
  void OptSetGradient(const SplitIndexTPST<TenElemT> &g) { check_rc(pepsgpu_opt_set_gradient(ctx_, dptr(g.flat().data())), ctx_); }
  void OptGetGradient(SplitIndexTPST<TenElemT> &g) const { check_rc(pepsgpu_opt_get_gradient(ctx_, dptr(g.flat().data())), ctx_); }
  double OptClip(double clip_value, double clip_norm) {
    double nrm = 0.0;
    check_rc(pepsgpu_opt_clip(ctx_, clip_value, clip_norm, &nrm), ctx_);
    return nrm;
  }
  struct NaturalGradientInfo { double residual_norm = 0.0, direction_norm = 0.0; int iterations = 0, reason = 0; };
  NaturalGradientInfo OptNaturalGradient(double diag_shift, size_t max_iter, double relative_tolerance, double absolute_tolerance,
                                         int residual_recompute_interval, double orthogonality_threshold) {
    NaturalGradientInfo r;
    check_rc(pepsgpu_opt_natural_gradient(ctx_, diag_shift, (int)max_iter, relative_tolerance, absolute_tolerance, residual_recompute_interval,
                                          orthogonality_threshold, &r.residual_norm, &r.iterations, &r.reason, &r.direction_norm), ctx_);
    return r;
  }
  // g <- the MinSR direction of the sample store (pepsgpu_minsr_direction): Gram, centering, eigensolve, cutoff and back-substitution on
  // the device; energy_samples in the order the samples were appended
  struct MinSRInfo { double direction_norm = 0.0, lambda_max = 0.0, cutoff = 0.0; size_t n_kept = 0, sweeps = 0; };
  MinSRInfo MinSRDirection(const std::vector<TenElemT> &energy_samples, const TenElemT &energy, double r_pinv, double a_pinv, bool soft_cutoff) {
    MinSRInfo r;
    double info[4] = {0.0, 0.0, 0.0, 0.0};
    check_rc(pepsgpu_minsr_direction(ctx_, dptr(energy_samples.data()), dptr(&energy), r_pinv, a_pinv, soft_cutoff ? 1 : 0, &r.direction_norm, info),
             ctx_);
    r.lambda_max = info[0]; r.cutoff = info[1]; r.n_kept = (size_t)info[2]; r.sweeps = (size_t)info[3];
    return r;
  }
  size_t SRCount() const { const int n = pepsgpu_sr_count(ctx_); return n > 0 ? (size_t)n : 0; }
  void OptStep(int rule, double lr, const std::vector<double> &params) {
    check_rc(pepsgpu_opt_step(ctx_, rule, lr, params.data(), (int)params.size()), ctx_);
  }
  void OptScaleState(double factor) { check_rc(pepsgpu_opt_scale_state(ctx_, factor), ctx_); }
  // the base of a step, kept in HBM (pepsgpu_guard_*): prev_accepted_state_ of the spike rollback and the base of the selector trials
  void OptBaseSave() { check_rc(pepsgpu_guard_base_save(ctx_), ctx_); }
  void OptBaseRestore() { check_rc(pepsgpu_guard_base_restore(ctx_), ctx_); }
  void OptBaseClear() { check_rc(pepsgpu_guard_base_clear(ctx_), ctx_); }
  // theta <- the SGD rule on (base, g, velocity), the velocity untouched; params (0, 0, 0): base - lr g
  void OptPreview(double lr, const std::vector<double> &params) {
    check_rc(pepsgpu_guard_preview(ctx_, 0, lr, params.data(), (int)params.size()), ctx_);
  }
  // L-BFGS on the optimizer buffers (pepsgpu_lbfgs_*): history, anchor, direction and the base of the line search stay in HBM
  void LBFGSBegin(size_t history_size) { check_rc(pepsgpu_lbfgs_begin(ctx_, (int)std::min<size_t>(history_size, 1u << 20)), ctx_); }
  void LBFGSReset() { check_rc(pepsgpu_lbfgs_reset(ctx_), ctx_); }
  struct LBFGSUpdateInfo { int outcome = 0; double curvature = 0.0; };      // outcome: 0 no anchor, 1 pushed, 2 pushed after damping, 3 skipped
  LBFGSUpdateInfo LBFGSUpdate(double min_curvature, bool use_damping) {
    LBFGSUpdateInfo r;
    check_rc(pepsgpu_lbfgs_update(ctx_, min_curvature, use_damping ? 1 : 0, &r.outcome, &r.curvature), ctx_);
    return r;
  }
  struct LBFGSDirectionInfo { double dphi0 = 0.0, norm = 0.0; bool was_reset = false; };
  LBFGSDirectionInfo LBFGSDirection(double min_curvature, double max_direction_norm) {
    LBFGSDirectionInfo r;
    int reset = 0;
    check_rc(pepsgpu_lbfgs_direction(ctx_, min_curvature, max_direction_norm, &r.dphi0, &r.norm, &reset), ctx_);
    r.was_reset = reset != 0;
    return r;
  }
  void LBFGSTrial(double alpha) { check_rc(pepsgpu_lbfgs_trial(ctx_, alpha), ctx_); }
  double LBFGSSlope() { double d = 0.0; check_rc(pepsgpu_lbfgs_slope(ctx_, &d), ctx_); return d; }
  void LBFGSCommit() { check_rc(pepsgpu_lbfgs_commit(ctx_), ctx_); }
  void LBFGSGetDirection(SplitIndexTPST<TenElemT> &d) const { check_rc(pepsgpu_lbfgs_get_direction(ctx_, dptr(d.flat().data())), ctx_); }
  struct LBFGSCounters { size_t skip_curvature = 0, damping = 0, descent_reset = 0, history = 0; };
  LBFGSCounters LBFGSGetCounters() const {
    long c[4] = {0, 0, 0, 0};
    check_rc(pepsgpu_lbfgs_counters(ctx_, c), ctx_);
    return {(size_t)c[0], (size_t)c[1], (size_t)c[2], (size_t)c[3]};
  }
  void OptReadState(SplitIndexTPST<TenElemT> &s) const { check_rc(pepsgpu_opt_read_state(ctx_, dptr(s.flat().data())), ctx_); }
  // the lowest-energy parameters of a VMC run, kept in HBM (pepsgpu_vmc_snapshot_*): a device-to-device copy of theta
  void VMCSnapshotSave() { check_rc(pepsgpu_vmc_snapshot_save(ctx_), ctx_); }
  void VMCSnapshotRead(SplitIndexTPST<TenElemT> &s) const { check_rc(pepsgpu_vmc_snapshot_read(ctx_, dptr(s.flat().data())), ctx_); }
  void VMCSnapshotClear() { check_rc(pepsgpu_vmc_snapshot_clear(ctx_), ctx_); }
  void SRBegin(size_t max_samples) { check_rc(pepsgpu_sr_begin(ctx_, (int)max_samples), ctx_); }
  void SRAppend(const std::vector<TenElemT> &psi) { check_rc(pepsgpu_sr_append(ctx_, dptr(psi.data())), ctx_); }
  void UpdateLocal(const std::vector<int32_t> &sites, const std::vector<int32_t> &new_states, const std::vector<uint8_t> &mask) {
    check_rc(pepsgpu_update_local(ctx_, (int)(sites.size() / 2), sites.data(), new_states.data(), mask.data()), ctx_);
  }
  std::vector<TenElemT> EvaluateAmplitude() {
    std::vector<TenElemT> out(walkers());
    check_rc(pepsgpu_evaluate_amplitude(ctx_, dptr(out.data())), ctx_);
    return out;
  }
  std::vector<int32_t> WalkerFlags() const {
    std::vector<int32_t> f(walkers());
    check_rc(pepsgpu_walker_flags(ctx_, f.data()), ctx_);
    return f;
  }

 private:
  size_t rows_, cols_, D_, d_;
  BMPSTruncateParams trunc_;
  pepsgpu_ctx *ctx_ = nullptr;
};
using BMPSContractor = BMPSContractorT<double>;

// ---------------------------------------------------------------------------------------------
// Fermionic (fZ2-graded) states.  The graded contraction of the projected network equals an ordinary
// contraction of sign-decorated site tensors (peps_amd/fermion.py; proof obligations in
// tests/test_oracle_fermion.py), so a fermionic SplitIndexTPS is uploaded with 4 d "extended" components
// per site and every fermionic sign becomes the choice of a component: extended state = s + d * variant,
// variant 0/1 = row-major mode order with an even/odd number of fermions at sites <= v, variant 2/3 =
// column-major order with an even/odd number of fermions before v.  Nearest-neighbour hops along a row
// (column) are adjacent in the row-major (column-major) order: no Jordan-Wigner string, and only the
// extended states of the two sites change.
enum ModeOrder { ROW_MAJOR = 0, COL_MAJOR = 1 };
struct FermionDecoration {
  std::vector<int> nf;                         // fermion parity of each physical state (0 = occupied -> 1)
  // parity of every bond state, [rows][cols][4][D] (legs L, D, R, U; entries past a leg's dimension unused): what the
  // device-resident Optimizer needs to fold gradients and project in HBM (pepsgpu_fermion_decoration_set); empty elsewhere
  std::vector<uint8_t> bond_parity;
  size_t d() const { return nf.size(); }
  int n(int32_t state) const { return nf[(size_t)state] & 1; }
  // extended state of `site` for walker w, given the physical configuration
  int32_t Ext(const Configuration &cfg, size_t w, const SiteIdx &site, ModeOrder order) const {
    int par = 0;
    if (order == ROW_MAJOR) {
      for (size_t r = 0; r <= site.r; ++r)
        for (size_t c = 0; c < cfg.cols(); ++c) {
          if (r == site.r && c > site.c) break;
          par ^= n(cfg(w, {r, c}));
        }
      return cfg(w, site) + (int32_t)d() * par;
    }
    for (size_t c = 0; c <= site.c; ++c)
      for (size_t r = 0; r < cfg.rows(); ++r) {
        if (c == site.c && r >= site.r) break;
        par ^= n(cfg(w, {r, c}));
      }
    return cfg(w, site) + (int32_t)d() * (2 + par);
  }
  Configuration ExtConfig(const Configuration &cfg, ModeOrder order) const {
    Configuration e(cfg.walkers(), cfg.rows(), cfg.cols());
    for (size_t w = 0; w < cfg.walkers(); ++w) {
      int par = 0;
      if (order == ROW_MAJOR) {
        for (size_t r = 0; r < cfg.rows(); ++r)
          for (size_t c = 0; c < cfg.cols(); ++c) { par ^= n(cfg(w, {r, c})); e(w, {r, c}) = cfg(w, {r, c}) + (int32_t)d() * par; }
      } else {
        for (size_t c = 0; c < cfg.cols(); ++c)
          for (size_t r = 0; r < cfg.rows(); ++r) { e(w, {r, c}) = cfg(w, {r, c}) + (int32_t)d() * (2 + par); par ^= n(cfg(w, {r, c})); }
      }
    }
    return e;
  }
  // <S|Psi> (parity legs in row-major order) = Sigma * ordinary contraction of the row-major decorated network
  int Sigma(const Configuration &cfg, size_t w) const {
    long nfm = 0;
    for (size_t r = 0; r < cfg.rows(); ++r)
      for (size_t c = 0; c < cfg.cols(); ++c) nfm += n(cfg(w, {r, c}));
    return ((nfm + nfm * (nfm - 1) / 2) & 1) ? -1 : 1;
  }
  // sign of reordering the occupied (odd) modes from row-major to column-major order: the decorated contraction in the
  // column-major mode order gives the graded amplitude with the parity legs in column-major order, Kappa brings it to the
  // row-major convention every stored amplitude uses
  int Kappa(const Configuration &cfg, size_t w) const {
    std::vector<std::pair<size_t, size_t>> keys;          // (col, row) of the occupied sites, listed in row-major order
    for (size_t r = 0; r < cfg.rows(); ++r)
      for (size_t c = 0; c < cfg.cols(); ++c)
        if (n(cfg(w, {r, c}))) keys.emplace_back(c, r);
    size_t inv = 0;
    for (size_t i = 0; i < keys.size(); ++i)
      for (size_t j = i + 1; j < keys.size(); ++j) inv += keys[i] > keys[j];
    return (inv & 1) ? -1 : 1;
  }
};

// Triple table of the three-site exchange (pepsgpu_sweep_slice_tnn3, square_3site_updater.h:118-127): [dp^3][kTNN3Tab], entry
// e1 dp^2 + e2 dp + e3 = {m, init, six slots of three states}: the m distinct permutations of the sorted triple in
// std::next_permutation order, init the slot of the triple itself, unused slots repeating slot 0.  (The engine builds the bosonic
// table itself for a NULL table -- tnn3_boson_table of engine_sweep.h, the same rule; tests/test_cpu_tnn3.py pins the two together
// through pepsgpu_diag_tnn3_table.)
constexpr int kTNN3Tab = 20;
// the distinct permutations of t in std::next_permutation order of the sorted triple; *init = the slot of t itself; returns their number
inline int TNN3Permutations(const int32_t t[3], int32_t perm[6][3], int *init) {
  int32_t p[3] = {t[0], t[1], t[2]};
  std::sort(p, p + 3);
  int m = 0;
  do {
    if (p[0] == t[0] && p[1] == t[1] && p[2] == t[2]) *init = m;
    std::copy(p, p + 3, perm[m++]);
  } while (std::next_permutation(p, p + 3));
  return m;
}
inline void TNN3PutEntry(int32_t *row, int m, int init, const int32_t perm[6][3]) {
  row[0] = m;
  row[1] = init;
  for (int k = 0; k < 6; ++k) std::copy(perm[k < m ? k : 0], perm[k < m ? k : 0] + 3, row + 2 + 3 * k);
}
inline std::vector<int32_t> TNN3TripleTable(int dp) {      // bosonic states
  std::vector<int32_t> tab((size_t)dp * dp * dp * kTNN3Tab);
  for (int e = 0; e < dp * dp * dp; ++e) {
    const int32_t t[3] = {e / (dp * dp), (e / dp) % dp, e % dp};
    int32_t perm[6][3];
    int init = 0;
    const int m = TNN3Permutations(t, perm, &init);
    TNN3PutEntry(tab.data() + (size_t)e * kTNN3Tab, m, init, perm);
  }
  return tab;
}
// fermions: over the extended states (dp = 4 d) of three sites consecutive in `order`, the permutations of the PHYSICAL triple, each
// as extended states (the variants follow the parity before the first site, read off its extended state, as DeviceStatesRun does).
// A triple whose variants do not belong to `order`, or of three equal physical states, maps to itself alone.
inline std::vector<int32_t> FermionTNN3Table(const FermionDecoration &fd, ModeOrder order) {
  const int32_t d = (int32_t)fd.d(), dp = 4 * d;
  std::vector<int32_t> tab((size_t)dp * dp * dp * kTNN3Tab);
  for (int32_t e = 0; e < dp * dp * dp; ++e) {
    const int32_t ex[3] = {e / (dp * dp), (e / dp) % dp, e % dp};
    const int32_t ph[3] = {ex[0] % d, ex[1] % d, ex[2] % d};
    bool ok = true;
    for (int q = 0; q < 3; ++q) ok = ok && (order == ROW_MAJOR ? ex[q] / d < 2 : ex[q] / d >= 2);
    int32_t perm[6][3];
    int init = 0, m = 1;
    if (!ok || (ph[0] == ph[1] && ph[1] == ph[2])) {
      std::copy(ex, ex + 3, perm[0]);
    } else {
      m = TNN3Permutations(ph, perm, &init);
      const int var1 = ex[0] / d, before = order == ROW_MAJOR ? ((var1 & 1) ^ fd.n(ph[0])) : (var1 & 1);
      for (int k = 0; k < m; ++k) {
        int par = before;
        for (int q = 0; q < 3; ++q) {
          const int32_t a = perm[k][q];
          const int na = fd.n(a);
          perm[k][q] = order == ROW_MAJOR ? a + d * (par ^ na) : a + d * (2 + par);
          par ^= na;
        }
      }
    }
    TNN3PutEntry(tab.data() + (size_t)e * kTNN3Tab, m, init, perm);
  }
  return tab;
}

// TPSWaveFunctionComponent (wave_function_component.h:136-379), one entry per walker.  `config` is always the
// PHYSICAL configuration; for a fermionic state (`fermion` set) the device is given the extended states of the
// current mode order.
template <typename TenElemT>
struct TPSWaveFunctionComponentT {
  Configuration config;
  std::vector<TenElemT> amplitude;
  BMPSContractorT<TenElemT> &contractor;
  BMPSTruncateParams trun_para;
  const FermionDecoration *fermion = nullptr;
  ModeOrder order = ROW_MAJOR;

  TPSWaveFunctionComponentT(const SplitIndexTPST<TenElemT> &sitps, const Configuration &cfg, BMPSContractorT<TenElemT> &c,
                           const FermionDecoration *ferm = nullptr)
      : config(cfg), contractor(c), trun_para(c.GetTruncateParams()), fermion(ferm) {
    contractor.UploadState(sitps);
    InitDevice();                            // tn = TensorNetwork2D(sitps, config); contractor.Init(tn)  (:159-160)
    EvaluateAmplitude();                     // :161
  }
  // the state is already on the device (an optimizer step wrote it there, pepsgpu_opt_step): no upload
  struct ResidentState {};
  TPSWaveFunctionComponentT(ResidentState, const Configuration &cfg, BMPSContractorT<TenElemT> &c, const FermionDecoration *ferm = nullptr)
      : config(cfg), contractor(c), trun_para(c.GetTruncateParams()), fermion(ferm) {
    InitDevice();
    EvaluateAmplitude();
  }
  void InitDevice() { contractor.Init(fermion ? fermion->ExtConfig(config, order) : config); }
  // Row pass (horizontal bonds) <-> column pass (vertical bonds) of a sweep / an energy evaluation: a fermionic
  // network is decorated for the mode order in which the bonds of the pass are local; bosons: no-op.
  void SetOrder(ModeOrder o) {
    if (!fermion || o == order) return;
    order = o;
    InitDevice();
  }
  const std::vector<TenElemT> &EvaluateAmplitude() {      // :187-212
    if (fermion && order != ROW_MAJOR) SetOrder(ROW_MAJOR);
    amplitude = contractor.EvaluateAmplitude();
    auto flags = contractor.WalkerFlags();
    for (size_t w = 0; w < flags.size(); ++w)
      if (flags[w])
        throw std::runtime_error("BMPS::MultiplyMPOSVDCompress_: Empty tensor (walker " + std::to_string(w) +
                                 "). Configuration may have near-zero amplitude due to numerical degeneracy.");
    if (fermion)
      for (size_t w = 0; w < amplitude.size(); ++w) amplitude[w] *= double(fermion->Sigma(config, w));
    return amplitude;
  }
  // the same without the throw: flags[w] != 0 marks a walker whose contraction ran into an empty tensor (MonteCarloEngine's
  // TryConstructWavefunction_, monte_carlo_engine.h: a failed construction is a rescue case, not an abort)
  std::vector<int32_t> EvaluateAmplitudeNoThrow() {
    if (fermion && order != ROW_MAJOR) SetOrder(ROW_MAJOR);
    amplitude = contractor.EvaluateAmplitude();
    auto flags = contractor.WalkerFlags();
    if (fermion)
      for (size_t w = 0; w < amplitude.size(); ++w) amplitude[w] *= double(fermion->Sigma(config, w));
    return flags;
  }
  void ReplaceGlobalConfig(const Configuration &cfg) {   // :180-185
    config = cfg;
    InitDevice();
    EvaluateAmplitude();
  }
  // physical candidate states of a run of sites consecutive in the current mode order (a nearest-neighbour bond, or the three sites
  // of a row / column triple) -> device states; cand [walker][n_cand][sites.size()]
  std::vector<int32_t> DeviceStatesRun(const std::vector<SiteIdx> &sites, int n_cand, const std::vector<int32_t> &cand) const {
    if (!fermion) return cand;
    const size_t nw = config.walkers(), d = fermion->d(), len = sites.size();
    std::vector<int32_t> out(cand.size());
    for (size_t w = 0; w < nw; ++w) {
      // parity of the fermions before the first site in the current order (does not depend on the states of the run)
      const int32_t e1 = fermion->Ext(config, w, sites[0], order);
      const int var1 = e1 / (int32_t)d;                                   // 0/1 (row: inclusive) or 2/3 (col: before)
      const int before = order == ROW_MAJOR ? ((var1 & 1) ^ fermion->n(config(w, sites[0]))) : (var1 & 1);
      for (int k = 0; k < n_cand; ++k) {
        int par = before;
        for (size_t q = 0; q < len; ++q) {
          const size_t i = (w * n_cand + k) * len + q;
          const int32_t a = cand[i];
          const int na = fermion->n(a);
          out[i] = order == ROW_MAJOR ? a + (int32_t)d * (par ^ na) : a + (int32_t)d * (2 + par);
          par ^= na;
        }
      }
    }
    return out;
  }
  std::vector<int32_t> DeviceStatesNN(const SiteIdx &s1, const SiteIdx &s2, int n_cand, const std::vector<int32_t> &cand) const {
    return DeviceStatesRun({s1, s2}, n_cand, cand);
  }
  std::vector<TenElemT> ReplaceNNSiteTrace(const SiteIdx &s1, const SiteIdx &s2, BondOrientation dir, int n_cand,
                                         const std::vector<int32_t> &cand) const {
    return contractor.ReplaceNNSiteTrace(s1, dir, n_cand, DeviceStatesNN(s1, s2, n_cand, cand));
  }
  // Fermions: the exchange of two sites adjacent in the current mode order, DeviceStatesNN tabulated over the pair of extended states
  // (state + d * variant, dp = 4 d): the pair table [dp^2][2] of the device-side sweep and energy slices.  A pair whose variants do
  // not belong to the current order maps to itself.
  std::vector<int32_t> ExchangeTable() const {
    if (!fermion) throw std::logic_error("ExchangeTable: the component has no fermionic decoration");
    const FermionDecoration &fd = *fermion;
    const int32_t d = (int32_t)fd.d(), dp = 4 * d;
    std::vector<int32_t> tab((size_t)dp * dp * 2);
    for (int32_t e1 = 0; e1 < dp; ++e1)
      for (int32_t e2 = 0; e2 < dp; ++e2) {
        const int32_t a1 = e1 % d, var1 = e1 / d, a2 = e2 % d, var2 = e2 / d;
        int32_t c1 = e1, c2 = e2;
        const bool row_ok = order == ROW_MAJOR && var1 < 2 && var2 < 2, col_ok = order == COL_MAJOR && var1 >= 2 && var2 >= 2;
        if (row_ok || col_ok) {
          const int32_t a = a2, b = a1;                     // the exchanged physical states
          const int na = fd.n(a), nb = fd.n(b);
          const int before = row_ok ? ((var1 & 1) ^ fd.n(a1)) : (var1 & 1);
          if (row_ok) { c1 = a + d * (before ^ na); c2 = b + d * (before ^ na ^ nb); }
          else { c1 = a + d * (2 + before); c2 = b + d * (2 + (before ^ na)); }
        }
        tab[2 * ((size_t)e1 * dp + e2)] = c1;
        tab[2 * ((size_t)e1 * dp + e2) + 1] = c2;
      }
    return tab;
  }
  // Fermions: the three-site exchange of three sites consecutive in the current mode order, the triple table [dp^3][20] of
  // pepsgpu_sweep_slice_tnn3 over the extended states (dp = 4 d): the distinct permutations of the PHYSICAL triple in
  // std::next_permutation order, each as the extended states DeviceStatesRun gives it.  A triple whose variants do not belong to the
  // current order (or whose physical states are equal) maps to itself alone.
  std::vector<int32_t> TNN3Table() const {
    if (!fermion) throw std::logic_error("TNN3Table: the component has no fermionic decoration");
    return FermionTNN3Table(*fermion, order);
  }
  // UpdateLocal (:345-378) for the walkers with mask != 0; new_states are physical, [walker][site]
  void UpdateLocal(const std::vector<TenElemT> &new_amplitude, const std::vector<SiteIdx> &sites,
                   const std::vector<int32_t> &new_states, const std::vector<uint8_t> &mask) {
    std::vector<int32_t> flat_sites;
    for (auto &s : sites) { flat_sites.push_back((int32_t)s.r); flat_sites.push_back((int32_t)s.c); }
    if (fermion) {
      // (a run of sites consecutive in the current mode order: a nearest-neighbour pair, or a triple of a row / column)
      if (sites.size() != 2 && sites.size() != 3) throw std::invalid_argument("fermionic UpdateLocal: pairs or triples of consecutive sites only");
      contractor.UpdateLocal(flat_sites, DeviceStatesRun(sites, 1, new_states), mask);
    } else {
      contractor.UpdateLocal(flat_sites, new_states, mask);
    }
    for (size_t w = 0; w < mask.size(); ++w) {
      if (!mask[w]) continue;
      for (size_t k = 0; k < sites.size(); ++k) config(w, sites[k]) = new_states[w * sites.size() + k];
      // new_amplitude is the contraction value of the replace-trace: for a fermionic state that is the DECORATED network
      // of the current mode order; the stored amplitude is always the signed graded one (as EvaluateAmplitude stores it)
      amplitude[w] = fermion ? new_amplitude[w] * double(fermion->Sigma(config, w) * (order == COL_MAJOR ? fermion->Kappa(config, w) : 1))
                             : new_amplitude[w];
    }
  }
  bool IsAmplitudeSquareLegal(size_t w) const {          // :309-315
    double a = std::abs(amplitude[w]);
    return !std::isnan(a) && a > std::sqrt(std::numeric_limits<double>::min()) && a < std::sqrt(std::numeric_limits<double>::max());
  }
};
using TPSWaveFunctionComponent = TPSWaveFunctionComponentT<double>;

// suwa_todo_update.h:53-112
template <class RandGenerator>
size_t SuwaTodoStateUpdate(size_t init_state, std::vector<double> weights, RandGenerator &generator) {
  const size_t n = weights.size();
  auto max_it = std::max_element(weights.cbegin(), weights.cend());
  const size_t max_id = max_it - weights.cbegin();
  if (max_id != 0) std::swap(weights[0], weights[max_id]);
  if (init_state == max_id) init_state = 0;
  else if (init_state == 0) init_state = max_id;
  std::vector<long double> s(n);
  s[0] = weights[0];
  for (size_t i = 1; i < n; i++) s[i] = s[i - 1] + (long double)weights[i];
  const long double S = s.back();
  const long double s_im1 = (init_state == 0) ? 0.0L : s[init_state - 1];
  long double start = s_im1 + (long double)weights[0];
  if (start >= S) start -= S;
  std::uniform_real_distribution<long double> dist(start, std::nextafter(start + (long double)weights[init_state], start));
  long double x = dist(generator);
  if (x >= S) x -= S;
  size_t final_state = std::upper_bound(s.begin(), s.end(), x) - s.begin();
  if (final_state >= n) final_state = n - 1;
  if (max_id != 0) {
    if (final_state == 0) final_state = max_id;
    else if (final_state == max_id) final_state = 0;
  }
  return final_state;
}

// an updater opts into the device-side slice sweep with `static constexpr bool kDeviceSliceSweep = true` + SweepSliceOnDevice
template <typename U, typename = void> struct HasDeviceSliceSweep : std::false_type {};
template <typename U> struct HasDeviceSliceSweep<U, std::void_t<decltype(U::kDeviceSliceSweep)>> : std::bool_constant<U::kDeviceSliceSweep> {};

// PEPSHOST_NO_DEVICE_SWEEP=1 keeps the updaters and the energy solvers on their per-site / per-bond hook paths (A/B and the
// identical-chain tests of the two paths); read once per process
inline bool DeviceSlicesEnabled() {
  static const bool enabled = std::getenv("PEPSHOST_NO_DEVICE_SWEEP") == nullptr;
  return enabled;
}
// Does this updater run a whole row / column in ONE device call for this component?  (An updater whose move the device implements:
// traces, acceptance tests and moves on the device, the walker's random stream consumed in the same order -> the same chain.
// Every other combination goes through its hook, bond by bond.)
template <typename MCUpdater, typename TenElemT>
bool TakesDeviceSlicePath(const TPSWaveFunctionComponentT<TenElemT> &comp) {
  if constexpr (HasDeviceSliceSweep<MCUpdater>::value) return DeviceSlicesEnabled() && (!comp.fermion || MCUpdater::kDeviceSliceSweepFermions);
  else return false;
}

// one row (HORIZONTAL) or column (VERTICAL) of the lattice as a sweep walks it: N sites at(0) .. at(N - 1), the BTen that grows (lo)
// and the one that shrinks (hi)
struct SliceSites {
  BondOrientation dir;
  size_t num, N;
  template <typename Contractor>
  SliceSites(const Contractor &c, BondOrientation dir_, size_t num_) : dir(dir_), num(num_), N(dir_ == HORIZONTAL ? c.cols() : c.rows()) {}
  SiteIdx at(size_t j) const { return dir == HORIZONTAL ? SiteIdx{num, j} : SiteIdx{j, num}; }
  BTenPOSITION lo() const { return dir == HORIZONTAL ? LEFT : UP; }
  BTenPOSITION hi() const { return dir == HORIZONTAL ? RIGHT : DOWN; }
};

// psi as a divisor: a zero amplitude is the error of the reference's solvers
template <typename TenElemT>
inline const TenElemT &NonZeroPsi(const TenElemT &psi) {
  if (psi == TenElemT(0.0)) throw std::runtime_error("Wavefunction amplitude is near zero, causing division by zero.");
  return psi;
}
template <typename TenElemT>
inline std::vector<TenElemT> InversePsi(const std::vector<TenElemT> &psi) {
  std::vector<TenElemT> inv(psi.size());
  for (size_t w = 0; w < psi.size(); ++w) inv[w] = TenElemT(1.0) / NonZeroPsi(psi[w]);
  return inv;
}

// Where the holes of a row pass go: nowhere (!wanted: the measurements), into HBM (on_device: PunchHoleStore), else conjugated --
// hole_res(site) = Dag(hole), square_nnn_energy_solver.h:163 -- into host [walker][row][col][slot], which is sized here
template <typename TenElemT>
struct HoleDest {
  bool wanted = false, on_device = false;
  size_t slot = 0;
  std::vector<TenElemT> *host = nullptr;
  HoleDest() = default;
  HoleDest(bool calchols, bool holes_on_device, size_t slot_, const TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &out)
      : wanted(calchols), on_device(holes_on_device), slot(slot_), host(&out) {
    if (wanted && !on_device) out.assign(comp.config.walkers() * comp.contractor.rows() * comp.contractor.cols() * slot, TenElemT(0.0));
  }
  // the hole of site s of the current row window
  void Punch(BMPSContractorT<TenElemT> &c, const SiteIdx &s) const {
    if (!wanted) return;
    if (on_device) { c.PunchHoleStore(s, HORIZONTAL); return; }
    const std::vector<TenElemT> h = c.PunchHole(s, HORIZONTAL);
    for (size_t w = 0; w * slot < h.size(); ++w)
      std::transform(h.begin() + w * slot, h.begin() + (w + 1) * slot, host->begin() + ((w * c.rows() + s.r) * c.cols() + s.c) * slot,
                     [](const TenElemT &x) { return ComplexConjugate(x); });
  }
};

// MonteCarloSweepUpdaterBase (monte_carlo_sweep_updater_base.h:18-47): one std::mt19937 per walker
class MonteCarloSweepUpdaterBase {
 public:
  explicit MonteCarloSweepUpdaterBase(const std::vector<uint64_t> &seeds) {
    for (auto s : seeds) engines_.emplace_back((std::mt19937::result_type)s);
  }
 protected:
  std::vector<std::mt19937> engines_;
  // Values drawn AHEAD of their use (a device-side slice sweep hands the next few of every walker's stream to the kernel, which
  // consumes a prefix): a walker's values are always taken from the front of its queue first, so the sequence it consumes is the
  // sequence draw(engines_[w]) yields -- whichever path (device slice, host hook) asks for the next one.
  template <typename V, typename Draw>         // Draw: V operator()(std::mt19937 &), one value off the engine
  class LookAhead {
   public:
    V Next(std::vector<std::mt19937> &engines, size_t w) {
      if (w < q_.size() && head_[w] < q_[w].size()) return q_[w][head_[w]++];
      return draw_(engines[w]);
    }
    // the next `cnt` values of every walker, [walker][cnt], without consuming them
    std::vector<V> PeekAll(std::vector<std::mt19937> &engines, size_t cnt) {
      if (q_.size() < engines.size()) { q_.resize(engines.size()); head_.resize(engines.size(), 0); }
      std::vector<V> out(engines.size() * cnt);
      for (size_t w = 0; w < engines.size(); ++w) {
        auto &q = q_[w];
        if (head_[w] > 0 && head_[w] == q.size()) { q.clear(); head_[w] = 0; }
        else if (head_[w] > 64) { q.erase(q.begin(), q.begin() + (long)head_[w]); head_[w] = 0; }
        while (q.size() - head_[w] < cnt) q.push_back(draw_(engines[w]));
        std::copy(q.begin() + (long)head_[w], q.begin() + (long)(head_[w] + cnt), out.begin() + (long)(w * cnt));
      }
      return out;
    }
    void Consume(size_t w, size_t cnt) { head_[w] += cnt; }
   private:
    std::vector<std::vector<V>> q_;            // [walker] drawn, not yet consumed (front = head_[w])
    std::vector<size_t> head_;
    Draw draw_;
  };
  struct DrawUniform {
    std::uniform_real_distribution<double> dist{0.0, 1.0};
    double operator()(std::mt19937 &e) { return dist(e); }
  };
  struct DrawWord { uint32_t operator()(std::mt19937 &e) { return (uint32_t)e(); } };
  // An updater draws either deviates or raw engine words, never both.
  LookAhead<double, DrawUniform> uniforms_;
  LookAhead<uint32_t, DrawWord> words_;
  double NextUniform(size_t w) { return uniforms_.Next(engines_, w); }
  uint32_t NextWord(size_t w) { return words_.Next(engines_, w); }
  // walker w's std::mt19937 with the queued words served first (a URBG with the engine's range: a distribution draws from it exactly
  // the words it would draw from the engine)
  struct QueuedEngine {
    using result_type = std::mt19937::result_type;
    MonteCarloSweepUpdaterBase *base;
    size_t w;
    static constexpr result_type min() { return std::mt19937::min(); }
    static constexpr result_type max() { return std::mt19937::max(); }
    result_type operator()() { return base->NextWord(w); }
  };
  QueuedEngine Engine(size_t w) { return QueuedEngine{this, w}; }

  // The schedule of a sweep (square_nn_updater.h:28-82, square_3site_updater.h:28-91): every row under the row-major mode order
  // (fermions: the W sites of a row window are consecutive modes of it), then every column under the column-major one.  A slice goes
  // to self->SweepSliceOnDevice when the updater takes the device path, else to hook_slice(sites, acc); both add a walker's accepted
  // moves to acc.  accept_rates = acc / the number of windows of W sites on the lattice.
  template <typename MCUpdater, typename TenElemT, typename HookSlice>
  static void SweepRowsThenColumns(MCUpdater *self, const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp, size_t W,
                                   std::vector<double> &accept_rates, HookSlice &&hook_slice) {
    auto &c = comp.contractor;
    const size_t rows = c.rows(), cols = c.cols(), n = comp.config.walkers();
    std::vector<size_t> acc(n, 0);
    const bool dev_slice = TakesDeviceSlicePath<MCUpdater>(comp);
    auto slice = [&](BondOrientation dir, size_t num) {
      if (!dev_slice) hook_slice(SliceSites(c, dir, num), acc);
      else if constexpr (HasDeviceSliceSweep<MCUpdater>::value) self->SweepSliceOnDevice(dir, num, sitps, comp, acc);
    };
    comp.SetOrder(ROW_MAJOR);
    c.GenerateBMPSApproach(UP);
    for (size_t row = 0; row < rows; row++) {
      slice(HORIZONTAL, row);
      if (row + 1 < rows) c.ShiftBMPSWindow(DOWN);
    }
    c.DeleteInnerBMPS(LEFT);
    c.DeleteInnerBMPS(RIGHT);
    comp.SetOrder(COL_MAJOR);
    c.GenerateBMPSApproach(LEFT);
    for (size_t col = 0; col < cols; col++) {
      slice(VERTICAL, col);
      if (col + 1 < cols) c.ShiftBMPSWindow(RIGHT);
    }
    c.DeleteInnerBMPS(UP);
    const double total = double(cols * (rows - (W - 1)) + rows * (cols - (W - 1)));
    accept_rates.assign(n, 0.0);
    for (size_t w = 0; w < n; ++w) accept_rates[w] = double(acc[w]) / total;
  }
  // what a device slice returned into the component: the states of the slice [walker][N] (fermions: extended states, taken % d) and
  // the accepted moves of every walker
  template <typename TenElemT>
  static void StoreSlice(TPSWaveFunctionComponentT<TenElemT> &comp, BondOrientation dir, size_t slice, const std::vector<int32_t> &states,
                         const std::vector<int32_t> &accepted, std::vector<size_t> &acc) {
    const SliceSites s(comp.contractor, dir, slice);
    const int32_t d = comp.fermion ? (int32_t)comp.fermion->d() : 0;
    for (size_t w = 0; w < acc.size(); ++w) {
      acc[w] += (size_t)accepted[w];
      for (size_t j = 0; j < s.N; ++j) comp.config(w, s.at(j)) = d ? states[w * s.N + j] % d : states[w * s.N + j];
    }
  }
  // the factor from a contraction of the decorated network of the current mode order to the stored (graded, row-major) amplitude
  template <typename TenElemT>
  static double GradedSign(const TPSWaveFunctionComponentT<TenElemT> &comp, size_t w) {
    if (!comp.fermion) return 1.0;
    return double(comp.fermion->Sigma(comp.config, w) * (comp.order == COL_MAJOR ? comp.fermion->Kappa(comp.config, w) : 1));
  }
};

// a model opts into the device-side energy slice with `static constexpr bool kExchangeBondEnergy = true` + the scalar hook
// TenElemT BondEnergyFromExchange(config1, config2, ratio), ratio = ComplexConjugate(psi_exchanged / psi) as its EvaluateBondEnergy
// forms it.  `kExchangeBondPsiPerBond = true`: its EvaluateBondEnergy divides by a Trace of the bond's own window (the fermionic
// models) -- the slice returns that psi per bond, and fermionic components are admitted (the exchange as the pair table).
template <typename U, typename = void> struct HasExchangeBondEnergy : std::false_type {};
template <typename U> struct HasExchangeBondEnergy<U, std::void_t<decltype(U::kExchangeBondEnergy)>> : std::bool_constant<U::kExchangeBondEnergy> {};
template <typename U, typename = void> struct HasExchangeBondPsiPerBond : std::false_type {};
template <typename U> struct HasExchangeBondPsiPerBond<U, std::void_t<decltype(U::kExchangeBondPsiPerBond)>> : std::bool_constant<U::kExchangeBondPsiPerBond> {};

// A fermionic model whose bond term is up to two hops (the Hubbard model) opts into the device-side slice with `static constexpr bool
// kHopBondEnergy = true`, HopTable() (the hop_table of pepsgpu_nn_hop_slice_fermion over its physical states) and the scalar hook
// TenElemT BondEnergyFromHops(config1, config2, r_up, r_dn), r = ComplexConjugate(psi'_k / psi) of the two candidate slots (0 where the
// bond has no such hop; psi'_k with Sigma(S') / Sigma(S) applied, as the slice returns it): one pepsgpu_nn_hop_slice_fermion per row and per column, the holes with the row slice when they are resident.
template <typename U, typename = void> struct HasHopBondEnergy : std::false_type {};
template <typename U> struct HasHopBondEnergy<U, std::void_t<decltype(U::kHopBondEnergy)>> : std::bool_constant<U::kHopBondEnergy> {};

// `kExchangeNNNEnergy = true` + the scalar hook NNNEnergyFromExchange(config1, config2, ratio), the twin of BondEnergyFromExchange
// for a diagonal link: the diagonal bonds of a row pair come from ONE pepsgpu_nnn_exchange_slice call.  `kNNNDiagMask` (optional, bit 0
// LEFTUP_TO_RIGHTDOWN, bit 1 LEFTDOWN_TO_RIGHTUP; default both) names the diagonals that interact: the others contribute exactly 0.
template <typename U, typename = void> struct HasExchangeNNNEnergy : std::false_type {};
template <typename U> struct HasExchangeNNNEnergy<U, std::void_t<decltype(U::kExchangeNNNEnergy)>> : std::bool_constant<U::kExchangeNNNEnergy> {};
template <typename U, typename = void> struct NNNDiagMask : std::integral_constant<int, 3> {};
template <typename U> struct NNNDiagMask<U, std::void_t<decltype(U::kNNNDiagMask)>> : std::integral_constant<int, U::kNNNDiagMask> {};

// The diagonal bonds of the row pair (row, row + 1) from the device slice (square_nnn_energy_solver.h:203-265 in one call): sink(w, col,
// e1, e2) gets, per walker and plaquette, what EvaluateNNNEnergy returns for LEFTUP_TO_RIGHTDOWN and LEFTDOWN_TO_RIGHTUP.  The BMPS
// pair of the row must be in place (the row pass before ShiftBMPSWindow(DOWN)); the BTen2 stacks end as the hook loop leaves them.
template <class Model, typename TenElemT, class Sink>
void NNNSliceEnergies(Model &model, TPSWaveFunctionComponentT<TenElemT> &comp, size_t row, const std::vector<TenElemT> &inv_psi, Sink &&sink) {
  auto &c = comp.contractor;
  const size_t n = comp.config.walkers(), np = c.cols() - 1;
  constexpr int mask = NNNDiagMask<Model>::value;
  std::vector<TenElemT> val(n * np * 2);
  check_rc(pepsgpu_nnn_exchange_slice(c.ctx(), (int)row, mask, dptr(val.data())), c.ctx());
  for (size_t w = 0; w < n; ++w)
    for (size_t col = 0; col < np; ++col) {
      const TenElemT *v = &val[(w * np + col) * 2];
      TenElemT e1(0.0), e2(0.0);
      if constexpr ((mask & 1) != 0)
        e1 = model.NNNEnergyFromExchange(comp.config(w, {row, col}), comp.config(w, {row + 1, col + 1}), ComplexConjugate(TenElemT(v[0] * inv_psi[w])));
      if constexpr ((mask & 2) != 0)
        e2 = model.NNNEnergyFromExchange(comp.config(w, {row + 1, col}), comp.config(w, {row, col + 1}), ComplexConjugate(TenElemT(v[1] * inv_psi[w])));
      sink(w, col, e1, e2);
    }
}
// The diagonal bonds of the row pair (row, row + 1), square_nnn_energy_solver.h:203-265: sink(w, col, e1, e2) as above, from ONE
// pepsgpu_nnn_exchange_slice (nnn_slice: a model with the scalar hook NNNEnergyFromExchange on a bosonic component; a fermionic diagonal hop
// keeps its twisted-environment path through the hooks), else from the hooks EvaluateNNNEnergy over the BTen2 of the pair.  Either way
// it needs the BMPS pair of the row and inv_psi only: unlike the NN slices it does not depend on where the holes go.
template <class Model, typename TenElemT, class Sink>
void NNNBondEnergies(Model &model, TPSWaveFunctionComponentT<TenElemT> &comp, bool nnn_slice, size_t row, const std::vector<TenElemT> &inv_psi,
                     Sink &&sink) {
  auto &c = comp.contractor;
  if (row + 1 >= c.rows()) return;
  if (nnn_slice) {
    if constexpr (HasExchangeNNNEnergy<Model>::value) NNNSliceEnergies(model, comp, row, inv_psi, sink);
    return;
  }
  c.InitBTen2(LEFT, row);
  c.GrowFullBTen2(RIGHT, row, 2, true);
  for (size_t col = 0; col + 1 < c.cols(); col++) {
    const std::vector<TenElemT> e1 = model.EvaluateNNNEnergy({row, col}, {row + 1, col + 1}, LEFTUP_TO_RIGHTDOWN, comp, inv_psi);
    const std::vector<TenElemT> e2 = model.EvaluateNNNEnergy({row + 1, col}, {row, col + 1}, LEFTDOWN_TO_RIGHTUP, comp, inv_psi);
    for (size_t w = 0; w < e1.size(); ++w) sink(w, col, e1[w], e2[w]);   // LEFTDOWN anchor mapped to the top cell (:155)
    c.ShiftBTen2Window(RIGHT, row);
  }
}

// What ONE device call returned for the np = N - 1 bonds of a row / column: psi [walker] -- [walker][np] when the slice reports the psi of
// every bond's own window (per_bond) --, the exchanged amplitude of every bond ex [walker][np], and two further candidates per bond
// two [walker][np][2]: the hops of pepsgpu_nn_hop_slice_fermion, the pair candidates of pepsgpu_nn_pair_slice_fermion
template <typename TenElemT>
struct BondSlice {
  size_t n, np;
  bool per_bond;
  std::vector<TenElemT> psi, ex, two;
  BondSlice(size_t n_, const SliceSites &s, bool per_bond_, bool with_ex, bool with_two)
      : n(n_), np(s.N - 1), per_bond(per_bond_), psi(per_bond_ ? n_ * np : n_), ex(with_ex ? n_ * np : 0), two(with_two ? n_ * np * 2 : 0) {}
  const TenElemT &Psi(size_t w, size_t j) const { return psi[per_bond ? w * np + j : w]; }
  // psi of the slice (per bond: the first bond's window is the slice's first window)
  std::vector<TenElemT> Psi0() const {
    std::vector<TenElemT> psi0(n);
    for (size_t w = 0; w < n; ++w) psi0[w] = per_bond && np == 0 ? TenElemT(1.0) : Psi(w, 0);
    return psi0;
  }
};
inline std::vector<int32_t> OccupationTable(const FermionDecoration &fd) {
  std::vector<int32_t> occ(fd.d());
  for (size_t s = 0; s < occ.size(); ++s) occ[s] = fd.n((int32_t)s);
  return occ;
}
// pepsgpu_nn_exchange_slice_tab: psi, the exchanged amplitude of every bond and -- holes: resident in HBM -- the holes of the row, one
// read-back, instead of a ReplaceNNSiteTrace round trip per bond.  Real and complex; a fermionic component through its ExchangeTable.
template <typename TenElemT>
BondSlice<TenElemT> ExchangeSlice(TPSWaveFunctionComponentT<TenElemT> &comp, const SliceSites &s, bool holes, bool per_bond) {
  auto &c = comp.contractor;
  BondSlice<TenElemT> sl(comp.config.walkers(), s, per_bond, true, false);
  const std::vector<int32_t> tab = comp.fermion ? comp.ExchangeTable() : std::vector<int32_t>();
  check_rc(pepsgpu_nn_exchange_slice_tab(c.ctx(), s.dir, (int)s.num, holes ? 1 : 0, tab.empty() ? nullptr : tab.data(), per_bond ? 1 : 0,
                                         dptr(sl.psi.data()), dptr(sl.ex.data())), c.ctx());
  return sl;
}
// pepsgpu_nn_hop_slice_fermion: psi per bond and the two hops of hop_table of every bond (the holes with a row when they are resident)
template <typename TenElemT>
BondSlice<TenElemT> HopSlice(TPSWaveFunctionComponentT<TenElemT> &comp, const SliceSites &s, bool holes, const std::vector<int32_t> &hop_table) {
  auto &c = comp.contractor;
  BondSlice<TenElemT> sl(comp.config.walkers(), s, true, false, true);
  const std::vector<int32_t> occ = OccupationTable(*comp.fermion);
  check_rc(pepsgpu_nn_hop_slice_fermion(c.ctx(), s.dir, (int)s.num, holes ? 1 : 0, (int)occ.size(), occ.data(), hop_table.data(), dptr(sl.psi.data()),
                                        dptr(sl.two.data())), c.ctx());
  return sl;
}
// pepsgpu_nn_pair_slice_fermion: psi per bond, the exchanged amplitude and the two pair candidates of pair_table of every bond
template <typename TenElemT>
BondSlice<TenElemT> PairSlice(TPSWaveFunctionComponentT<TenElemT> &comp, const SliceSites &s, const std::vector<int32_t> &pair_table) {
  auto &c = comp.contractor;
  BondSlice<TenElemT> sl(comp.config.walkers(), s, true, true, true);
  const std::vector<int32_t> occ = OccupationTable(*comp.fermion), xtab = comp.ExchangeTable();
  check_rc(pepsgpu_nn_pair_slice_fermion(c.ctx(), s.dir, (int)s.num, (int)occ.size(), occ.data(), pair_table.data(), xtab.data(), dptr(sl.psi.data()),
                                         dptr(sl.ex.data()), dptr(sl.two.data())), c.ctx());
  return sl;
}

// How the solvers of the square-lattice models evaluate NN bond j of a slice, per walker: e = the bond energy and, with_sc (the fermionic
// registry of a model with enable_sc_measurement), sc = the registry value (conj(delta_dag) + delta) / 2 of the bond-singlet pairing.
//   Read + FromSlice  the model's device slice: BondEnergyFromHops on the hop slice (kHopBondEnergy), else BondEnergyFromExchange on the
//                     exchange slice, psi per bond for kExchangeBondPsiPerBond -- pair_slice (the fermionic registry): on the pair slice,
//                     which also serves BondSCFromPairs with rho(S') = sign ReplaceNNSiteTrace / Trace from the same read-back;
//   Hook              EvaluateBondEnergy / EvaluateBondSC, a ReplaceNNSiteTrace round trip per bond.
template <typename TenElemT> struct BondValues { std::vector<TenElemT> e, sc; };
template <class Model, typename TenElemT, bool pair_slice, bool with_sc>
struct SquareModelBonds {
  Model &model;
  TPSWaveFunctionComponentT<TenElemT> &comp;
  std::vector<int32_t> pair_table;
  SquareModelBonds(Model &model_, TPSWaveFunctionComponentT<TenElemT> &comp_) : model(model_), comp(comp_) {
    if constexpr (with_sc) pair_table = model.PairTable();
    else if constexpr (pair_slice) pair_table.assign(4 * comp.fermion->d() * comp.fermion->d(), -1);
  }
  BondSlice<TenElemT> Read(const SliceSites &s, bool holes) const {
    if constexpr (HasHopBondEnergy<Model>::value) return HopSlice(comp, s, holes, model.HopTable());
    else if constexpr (pair_slice) return PairSlice(comp, s, pair_table);
    else return ExchangeSlice(comp, s, holes, HasExchangeBondPsiPerBond<Model>::value);
  }
  BondValues<TenElemT> FromSlice(const SliceSites &s, size_t j, const BondSlice<TenElemT> &sl, const std::vector<TenElemT> &inv_psi) const {
    BondValues<TenElemT> v{std::vector<TenElemT>(sl.n), std::vector<TenElemT>(with_sc ? sl.n : 0)};
    for (size_t w = 0; w < sl.n; ++w) {
      const int32_t c1 = comp.config(w, s.at(j)), c2 = comp.config(w, s.at(j + 1));
      const size_t k = w * sl.np + j;
      if constexpr (HasHopBondEnergy<Model>::value) {
        const TenElemT psi = NonZeroPsi(sl.Psi(w, j));
        v.e[w] = model.BondEnergyFromHops(c1, c2, ComplexConjugate(TenElemT(sl.two[2 * k] / psi)), ComplexConjugate(TenElemT(sl.two[2 * k + 1] / psi)));
      } else if constexpr (HasExchangeBondEnergy<Model>::value) {
        v.e[w] = model.BondEnergyFromExchange(c1, c2, sl.per_bond ? ComplexConjugate(TenElemT(sl.ex[k] / NonZeroPsi(sl.Psi(w, j))))
                                                                   : ComplexConjugate(TenElemT(sl.ex[k] * inv_psi[w])));
        if constexpr (with_sc) {
          const auto dd = model.BondSCFromPairs(c1, c2, TenElemT(sl.two[2 * k] / sl.Psi(w, j)), TenElemT(sl.two[2 * k + 1] / sl.Psi(w, j)));
          v.sc[w] = (ComplexConjugate(dd.first) + dd.second) / TenElemT(2.0);
        }
      } else {
        throw std::logic_error("the model has no device-side bond slice");
      }
    }
    return v;
  }
  BondValues<TenElemT> Hook(const SliceSites &s, size_t j, const std::vector<TenElemT> &inv_psi) const {
    BondValues<TenElemT> v{model.EvaluateBondEnergy(s.at(j), s.at(j + 1), s.dir, comp, inv_psi), {}};
    if constexpr (with_sc) {
      for (const auto &dd : model.EvaluateBondSC(s.at(j), s.at(j + 1), s.dir, comp))
        v.sc.push_back((ComplexConjugate(dd.first) + dd.second) / TenElemT(2.0));
    }
    return v;
  }
};

// The bond traversal of the energy and measurement solvers (square_nnn_energy_solver.h:116-200 + BondTraversalMixin::TraverseVerticalBonds,
// bond_traversal_mixin.h:113-144): every row under the row-major mode order (fermions: the two sites of a bond are adjacent modes of
// its pass, and the holes are those of the row-major decorated network), then every column under the column-major one.
//   dev_slice   a row / column is ONE device call, bonds.Read(sites, holes), evaluated by bonds.FromSlice(sites, j, slice, inv_psi):
//               the same operations in the same order on the device as the hook pass, same numbers.  The caller decides; wherever
//               PEPSHOST_NO_DEVICE_SWEEP=1 (DeviceSlicesEnabled()) enters its condition, that keeps the hook pass;
//   else        the hook pass: Trace, then bonds.Hook(sites, j, inv_psi) per bond, in a row behind the hole of every site.  A row
//               shifts the BTen window behind every bond, the last included; a column only while a bond follows.
// on_bond(sites, j, value) gets every bond in traversal order, after_slice(sites, inv_psi) runs before the BMPS window moves on (the
// diagonal bonds and links of a row pair / column pair hang there), before_rows() between GenerateBMPSApproach(UP) and the first row.
// Returns psi of every row and column in that order.
struct NoOp { void operator()() const {} };
template <typename TenElemT, class Bonds, class OnBond, class AfterSlice, class BeforeRows = NoOp>
std::vector<std::vector<TenElemT>> TraverseNNBonds(TPSWaveFunctionComponentT<TenElemT> &comp, bool dev_slice, const HoleDest<TenElemT> &holes,
                                                   const Bonds &bonds, OnBond &&on_bond, AfterSlice &&after_slice,
                                                   BeforeRows &&before_rows = BeforeRows()) {
  auto &c = comp.contractor;
  std::vector<std::vector<TenElemT>> psi_list;
  auto pass = [&](const SliceSites &s) {
    const bool row = s.dir == HORIZONTAL;
    std::vector<TenElemT> inv_psi;
    if (dev_slice) {
      const auto sl = bonds.Read(s, row && holes.wanted);
      psi_list.push_back(sl.Psi0());
      inv_psi = InversePsi(psi_list.back());
      for (size_t j = 0; j + 1 < s.N; ++j) on_bond(s, j, bonds.FromSlice(s, j, sl, inv_psi));
    } else {
      c.InitBTen(s.lo(), s.num);                                             // :142
      c.GrowFullBTen(s.hi(), s.num, row ? 1 : 2, true);                      // :143
      psi_list.push_back(c.Trace(s.at(0), s.dir));                           // :147
      inv_psi = InversePsi(psi_list.back());
      for (size_t j = 0; j < s.N; ++j) {
        if (row) holes.Punch(c, s.at(j));                                    // :163
        if (j + 1 == s.N) break;
        on_bond(s, j, bonds.Hook(s, j, inv_psi));
        if (row || j + 2 < s.N) c.ShiftBTenWindow(s.hi());                   // :200
      }
    }
    after_slice(s, inv_psi);
  };
  comp.SetOrder(ROW_MAJOR);
  c.GenerateBMPSApproach(UP);                                                // :116
  before_rows();
  for (size_t row = 0; row < c.rows(); row++) {
    pass(SliceSites(c, HORIZONTAL, row));
    if (row + 1 < c.rows()) c.ShiftBMPSWindow(DOWN);                         // :126
  }
  comp.SetOrder(COL_MAJOR);
  c.GenerateBMPSApproach(LEFT);                                              // bond_traversal_mixin.h:120
  for (size_t col = 0; col < c.cols(); col++) {
    pass(SliceSites(c, VERTICAL, col));
    if (col + 1 < c.cols()) c.ShiftBMPSWindow(RIGHT);
  }
  return psi_list;
}

// square_nn_updater.h:25-83: sweep schedule, CRTP hook TwoSiteNNUpdateLocalImpl(site1, site2, dir, sitps, comp) -> accepted[w]
template <typename MCUpdater>
class MCUpdateSquareNNUpdateBaseOBC : public MonteCarloSweepUpdaterBase {
 public:
  using MonteCarloSweepUpdaterBase::MonteCarloSweepUpdaterBase;
  template <typename TenElemT>
  void operator()(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<double> &accept_rates) {
    auto &c = comp.contractor;
    auto *self = static_cast<MCUpdater *>(this);
    // the device path: the exchange updater (pepsgpu_sweep_slice_exchange, real and complex states; fermionic ones through the
    // tabulated move of pepsgpu_sweep_slice_exchange_tab) and the full-space updater (pepsgpu_sweep_slice_fullspace, bosonic states)
    SweepRowsThenColumns(self, sitps, comp, 2, accept_rates, [&](const SliceSites &s, std::vector<size_t> &acc) {
      c.InitBTen(s.lo(), s.num);
      c.GrowFullBTen(s.hi(), s.num, 2, true);
      for (size_t j = 0; j + 1 < s.N; ++j) {
        const std::vector<uint8_t> a = self->TwoSiteNNUpdateLocalImpl(s.at(j), s.at(j + 1), s.dir, sitps, comp);
        for (size_t w = 0; w < acc.size(); ++w) acc[w] += a[w];
        if (j + 2 < s.N) c.ShiftBTenWindow(s.hi());
      }
    });
  }
};

// square_nn_updater.h:142-189
class MCUpdateSquareNNExchangeOBC : public MCUpdateSquareNNUpdateBaseOBC<MCUpdateSquareNNExchangeOBC> {
 public:
  using MCUpdateSquareNNUpdateBaseOBC<MCUpdateSquareNNExchangeOBC>::MCUpdateSquareNNUpdateBaseOBC;
  static constexpr bool kDeviceSliceSweep = true;
  static constexpr bool kDeviceSliceSweepFermions = true;
  // one row / column of exchange moves on the device (pepsgpu_sweep_slice_exchange / _tab); walker w consumes the next consumed[w]
  // deviates of its stream, exactly those TwoSiteNNUpdateLocalImpl would draw
  template <typename TenElemT>
  void SweepSliceOnDevice(BondOrientation dir, size_t slice, const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp,
                          std::vector<size_t> &acc) {
    auto &c = comp.contractor;
    const size_t n = comp.config.walkers(), N = dir == HORIZONTAL ? c.cols() : c.rows(), nu = N - 1;
    const std::vector<double> uni = uniforms_.PeekAll(engines_, nu);
    std::vector<int32_t> consumed(n), accepted(n), states(n * N);
    std::vector<TenElemT> amp = comp.amplitude;
    // Fermions: the device holds extended states (state + d * variant) of the current mode order; the exchange of two sites adjacent
    // in that order is DeviceStatesNN tabulated over the pair of extended states.  The slice returns decorated amplitudes (the
    // Metropolis test sees moduli only); a walker that moved gets its signs back from its new configuration, as UpdateLocal does.
    if (!comp.fermion)
      check_rc(pepsgpu_sweep_slice_exchange(c.ctx(), dir, (int)slice, (int)nu, uni.data(), dptr(amp.data()), consumed.data(), accepted.data(),
                                            states.data()), c.ctx());
    else
      check_rc(pepsgpu_sweep_slice_exchange_tab(c.ctx(), dir, (int)slice, (int)nu, uni.data(), comp.ExchangeTable().data(), dptr(amp.data()),
                                                consumed.data(), accepted.data(), states.data()), c.ctx());
    StoreSlice(comp, dir, slice, states, accepted, acc);
    for (size_t w = 0; w < n; ++w) {
      uniforms_.Consume(w, (size_t)consumed[w]);
      if (!comp.fermion) comp.amplitude[w] = amp[w];
      else if (accepted[w] > 0) comp.amplitude[w] = amp[w] * GradedSign(comp, w);
    }
  }
  template <typename TenElemT>
  std::vector<uint8_t> TwoSiteNNUpdateLocalImpl(const SiteIdx &s1, const SiteIdx &s2, BondOrientation dir,
                                                const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp) {
    const size_t n = comp.config.walkers();
    std::vector<int32_t> cand(n * 2);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      cand[2 * w] = comp.config(w, s2);
      cand[2 * w + 1] = comp.config(w, s1);
      any |= cand[2 * w] != cand[2 * w + 1];
    }
    std::vector<uint8_t> exchange(n, 0);
    if (!any) return exchange;            // every walker has equal spins on the bond (:149-151)
    std::vector<TenElemT> psi_b = comp.ReplaceNNSiteTrace(s1, s2, dir, 1, cand);
    for (size_t w = 0; w < n; ++w) {
      if (comp.config(w, s1) == comp.config(w, s2)) continue;
      const double pa = std::abs(comp.amplitude[w]), pb = std::abs(psi_b[w]);
      if (pb >= pa) exchange[w] = 1;
      else {
        const double div = pb / pa;
        exchange[w] = NextUniform(w) < div * div;
      }
    }
    comp.UpdateLocal(psi_b, {s1, s2}, cand, exchange);
    return exchange;
  }
};

// square_nn_updater.h:253-293
class MCUpdateSquareNNFullSpaceUpdateOBC : public MCUpdateSquareNNUpdateBaseOBC<MCUpdateSquareNNFullSpaceUpdateOBC> {
 public:
  using MCUpdateSquareNNUpdateBaseOBC<MCUpdateSquareNNFullSpaceUpdateOBC>::MCUpdateSquareNNUpdateBaseOBC;
  static constexpr bool kDeviceSliceSweep = true;
  static constexpr bool kDeviceSliceSweepFermions = false;    // (the move ranges over physical states: the hook path keeps fermions)
  // one row / column of full-space moves on the device (pepsgpu_sweep_slice_fullspace): SuwaTodoStateUpdate draws a long double
  // from the walker's engine = two raw 32-bit words per bond, whatever the data -- handed over in drawing order
  template <typename TenElemT>
  void SweepSliceOnDevice(BondOrientation dir, size_t slice, const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp,
                          std::vector<size_t> &acc) {
    auto &c = comp.contractor;
    const size_t n = comp.config.walkers(), N = dir == HORIZONTAL ? c.cols() : c.rows(), nwd = 2 * (N - 1);
    std::vector<uint32_t> words(n * nwd);
    for (size_t w = 0; w < n; ++w)
      for (size_t k = 0; k < nwd; ++k) words[w * nwd + k] = (uint32_t)engines_[w]();
    std::vector<int32_t> accepted(n), states(n * N);
    check_rc(pepsgpu_sweep_slice_fullspace(c.ctx(), dir, (int)slice, (int)sitps.PhysicalDim(), words.data(), dptr(comp.amplitude.data()),
                                           accepted.data(), states.data()), c.ctx());
    StoreSlice(comp, dir, slice, states, accepted, acc);
  }
  template <typename TenElemT>
  std::vector<uint8_t> TwoSiteNNUpdateLocalImpl(const SiteIdx &s1, const SiteIdx &s2, BondOrientation dir,
                                                const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp) {
    const size_t n = comp.config.walkers(), dim = sitps.PhysicalDim(), nc = dim * dim;
    std::vector<int32_t> cand(n * nc * 2);
    for (size_t w = 0; w < n; ++w)
      for (size_t k = 0; k < nc; ++k) { cand[(w * nc + k) * 2] = (int32_t)(k / dim); cand[(w * nc + k) * 2 + 1] = (int32_t)(k % dim); }
    std::vector<TenElemT> alt = comp.ReplaceNNSiteTrace(s1, s2, dir, (int)nc, cand);
    std::vector<uint8_t> changed(n, 0);
    std::vector<int32_t> ns(n * 2);
    std::vector<TenElemT> new_amp(n);
    for (size_t w = 0; w < n; ++w) {
      const size_t init = comp.config(w, s1) * dim + comp.config(w, s2);
      alt[w * nc + init] = comp.amplitude[w];
      std::vector<double> weights(nc);
      for (size_t k = 0; k < nc; ++k) weights[k] = AbsSquare(TenElemT(alt[w * nc + k] / comp.amplitude[w]));
      const size_t fin = SuwaTodoStateUpdate(init, weights, engines_[w]);
      changed[w] = fin != init;
      ns[2 * w] = (int32_t)(fin / dim); ns[2 * w + 1] = (int32_t)(fin % dim);
      new_amp[w] = alt[w * nc + fin];
    }
    comp.UpdateLocal(new_amp, {s1, s2}, ns, changed);
    return changed;
  }
};

// While alive, the per-bond Trace / ReplaceNNSiteTrace of the contractor scale their results in a kernel, as the device-side slices do
// (pepsgpu_trace_scaling): a hook path inside this scope returns the bits of the slice that replaces it.
template <typename TenElemT>
struct DeviceTraceScaling {
  pepsgpu_ctx *ctx;
  explicit DeviceTraceScaling(const BMPSContractorT<TenElemT> &c) : ctx(c.ctx()) { check_rc(pepsgpu_trace_scaling(ctx, 1), ctx); }
  ~DeviceTraceScaling() { (void)pepsgpu_trace_scaling(ctx, 0); }
  DeviceTraceScaling(const DeviceTraceScaling &) = delete;
  DeviceTraceScaling &operator=(const DeviceTraceScaling &) = delete;
};

// The single-site states of the Hubbard model (square_hubbard_model.h:18-45) and the two-site sectors of its U(1) x U(1) updater
// (square_hubbard_u1u1_updater.h:30-72)
enum class HubbardSingleSiteState { DoubleOccupancy, SpinUp, SpinDown, Empty };   // 0, 1, 2, 3
inline double HubbardConfig2Density(size_t config) {
  switch (HubbardSingleSiteState(config)) {
    case HubbardSingleSiteState::DoubleOccupancy: return 2;
    case HubbardSingleSiteState::SpinUp: return 1;
    case HubbardSingleSiteState::SpinDown: return 1;
    case HubbardSingleSiteState::Empty: return 0;
  }
  return -1;
}
inline double HubbardConfig2Spinz(size_t config) {
  switch (HubbardSingleSiteState(config)) {
    case HubbardSingleSiteState::SpinUp: return 0.5;
    case HubbardSingleSiteState::SpinDown: return -0.5;
    case HubbardSingleSiteState::DoubleOccupancy: case HubbardSingleSiteState::Empty: return 0;
  }
  return -1;
}
inline std::pair<size_t, size_t> HubbardConfig2SpinCounts(size_t config) {      // (N_up, N_down)
  switch (HubbardSingleSiteState(config)) {
    case HubbardSingleSiteState::DoubleOccupancy: return {1, 1};
    case HubbardSingleSiteState::SpinUp: return {1, 0};
    case HubbardSingleSiteState::SpinDown: return {0, 1};
    case HubbardSingleSiteState::Empty: return {0, 0};
  }
  throw std::invalid_argument("Invalid Hubbard configuration: " + std::to_string(config));
}
inline std::vector<std::pair<size_t, size_t>> EnumerateHubbardTwoSiteConfigsWithU1U1(size_t n_up_total, size_t n_down_total) {
  std::vector<std::pair<size_t, size_t>> result;
  for (size_t c1 = 0; c1 < 4; ++c1)
    for (size_t c2 = 0; c2 < 4; ++c2) {
      const auto n1 = HubbardConfig2SpinCounts(c1), n2 = HubbardConfig2SpinCounts(c2);
      if (n1.first + n2.first == n_up_total && n1.second + n2.second == n_down_total) result.emplace_back(c1, c2);
    }
  return result;
}
// The sector table of pepsgpu_sweep_slice_sector for the updater below, [16][2 + 2 * 4] over physical states: row a * 4 + b = {m, init,
// four slots (a', b')}: the sector of (a, b) in the enumeration order, init the slot of (a, b) itself, unused slots (-1, -1)
constexpr int kHubbardSlots = 4, kHubbardSectorRow = 2 + 2 * kHubbardSlots;
inline std::vector<int32_t> HubbardSectorTable() {
  std::vector<int32_t> tab(16 * kHubbardSectorRow, -1);
  for (size_t a = 0; a < 4; ++a)
    for (size_t b = 0; b < 4; ++b) {
      const auto na = HubbardConfig2SpinCounts(a), nb = HubbardConfig2SpinCounts(b);
      const auto valid = EnumerateHubbardTwoSiteConfigsWithU1U1(na.first + nb.first, na.second + nb.second);
      int32_t *row = tab.data() + (a * 4 + b) * kHubbardSectorRow;
      row[0] = (int32_t)valid.size();
      for (size_t k = 0; k < valid.size(); ++k) {
        row[2 + 2 * k] = (int32_t)valid[k].first;
        row[3 + 2 * k] = (int32_t)valid[k].second;
        if (valid[k].first == a && valid[k].second == b) row[1] = (int32_t)k;
      }
    }
  return tab;
}

// square_hubbard_u1u1_updater.h:90-158: per bond a Suwa-Todo choice among the pairs with the (N_up, N_down) of the bond
class MCUpdateSquareNNHubbardU1U1OBC : public MCUpdateSquareNNUpdateBaseOBC<MCUpdateSquareNNHubbardU1U1OBC> {
 public:
  using MCUpdateSquareNNUpdateBaseOBC<MCUpdateSquareNNHubbardU1U1OBC>::MCUpdateSquareNNUpdateBaseOBC;
  static constexpr bool kDeviceSliceSweep = true;
  static constexpr bool kDeviceSliceSweepFermions = true;   // (a move inside the sector keeps the fermion parity of the pair: local in the extended states)
  // one row / column on the device (pepsgpu_sweep_slice_sector): walker w consumes the next consumed[w] words of its engine, exactly
  // those TwoSiteNNUpdateLocalImpl would draw (two per bond whose sector has more than one state).  The slice returns decorated
  // amplitudes (the weights see moduli only); a walker that moved gets its signs back from its new configuration.
  template <typename TenElemT>
  void SweepSliceOnDevice(BondOrientation dir, size_t slice, const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp,
                          std::vector<size_t> &acc) {
    auto &c = comp.contractor;
    RequireHubbardStates(comp);
    const size_t n = comp.config.walkers(), N = dir == HORIZONTAL ? c.cols() : c.rows(), nwd = 2 * (N - 1);
    const std::vector<uint32_t> words = words_.PeekAll(engines_, nwd);
    std::vector<int32_t> consumed(n), accepted(n), states(n * N), occ;
    if (comp.fermion)
      for (int32_t s = 0; s < 4; ++s) occ.push_back(comp.fermion->n(s));
    std::vector<TenElemT> amp = comp.amplitude;
    check_rc(pepsgpu_sweep_slice_sector(c.ctx(), dir, (int)slice, 4, comp.fermion ? occ.data() : nullptr, kHubbardSlots, Table().data(), (int)nwd,
                                        words.data(), dptr(amp.data()), consumed.data(), accepted.data(), states.data()), c.ctx());
    StoreSlice(comp, dir, slice, states, accepted, acc);
    for (size_t w = 0; w < n; ++w) {
      words_.Consume(w, (size_t)consumed[w]);
      if (!comp.fermion) comp.amplitude[w] = amp[w];
      else if (accepted[w] > 0) comp.amplitude[w] = amp[w] * GradedSign(comp, w);
    }
  }
  // :95-157 batched over the walkers: ONE ReplaceNNSiteTrace over four fixed candidate slots, padded with the walker's own pair, so
  // that both paths hand the replacement trace the same operands; no trace and no draw when every walker's sector has one state
  template <typename TenElemT>
  std::vector<uint8_t> TwoSiteNNUpdateLocalImpl(const SiteIdx &s1, const SiteIdx &s2, BondOrientation dir,
                                                const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp) {
    RequireHubbardStates(comp);
    const size_t n = comp.config.walkers();
    const std::vector<int32_t> &tab = Table();
    std::vector<int32_t> cand(n * kHubbardSlots * 2), meta(n * 2);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      const int32_t a = comp.config(w, s1), b = comp.config(w, s2);
      const int32_t *row = tab.data() + (size_t)(a * 4 + b) * kHubbardSectorRow;
      for (int k = 0; k < kHubbardSlots; ++k) {
        cand[(w * kHubbardSlots + k) * 2] = k < row[0] ? row[2 + 2 * k] : a;
        cand[(w * kHubbardSlots + k) * 2 + 1] = k < row[0] ? row[3 + 2 * k] : b;
      }
      meta[2 * w] = row[0];
      meta[2 * w + 1] = row[1];
      any |= row[0] > 1;
    }
    std::vector<uint8_t> changed(n, 0);
    if (!any) return changed;                 // every walker's sector has one state (:114-116)
    const DeviceTraceScaling<TenElemT> scaling(comp.contractor);      // (the amplitudes of the slice, bit for bit)
    const std::vector<TenElemT> alt = comp.ReplaceNNSiteTrace(s1, s2, dir, kHubbardSlots, cand);
    std::vector<int32_t> ns(n * 2);
    std::vector<TenElemT> new_amp(n);
    for (size_t w = 0; w < n; ++w) {
      const int m = meta[2 * w], init = meta[2 * w + 1];
      if (m <= 1) continue;
      // |psi_k / psi|^2 as the kernel forms it (the ratio of the moduli, squared); the current state keeps its stored amplitude (:129)
      const double pa = std::abs(comp.amplitude[w]);
      std::vector<double> weights(m);
      for (int k = 0; k < m; ++k) {
        const double r = k == init ? 1.0 : std::abs(alt[w * kHubbardSlots + k]) / pa;
        weights[k] = r * r;
      }
      QueuedEngine eng = Engine(w);
      const int fin = (int)SuwaTodoStateUpdate((size_t)init, weights, eng);
      if (fin == init) continue;
      changed[w] = 1;
      ns[2 * w] = cand[(w * kHubbardSlots + fin) * 2];
      ns[2 * w + 1] = cand[(w * kHubbardSlots + fin) * 2 + 1];
      new_amp[w] = alt[w * kHubbardSlots + fin];
    }
    comp.UpdateLocal(new_amp, {s1, s2}, ns, changed);
    return changed;
  }

 private:
  template <typename TenElemT>
  static void RequireHubbardStates(const TPSWaveFunctionComponentT<TenElemT> &comp) {
    const size_t d = comp.fermion ? comp.fermion->d() : comp.contractor.phys_dim();
    if (d != 4) throw std::invalid_argument("MCUpdateSquareNNHubbardU1U1OBC: the state needs the four Hubbard states per site");
  }
  const std::vector<int32_t> &Table() {
    if (tab_.empty()) tab_ = HubbardSectorTable();
    return tab_;
  }
  std::vector<int32_t> tab_;
};
using MCUpdateSquareNNHubbardU1U1 = MCUpdateSquareNNHubbardU1U1OBC;   // the reference's backward-compatible alias

// square_3site_updater.h:22-93: sweep schedule of the three-site updaters, CRTP hook TNN3SiteUpdateImpl(site1, site2, site3, dir, sitps,
// comp) -> changed[w].  Every row (column) starts from the ReplaceTNNSiteTrace of its first window as the amplitude (:39-42, :64-67).
template <typename MCUpdater>
class MCUpdateSquareTNN3SiteUpdateBase : public MonteCarloSweepUpdaterBase {
 public:
  using MonteCarloSweepUpdaterBase::MonteCarloSweepUpdaterBase;
  template <typename TenElemT>
  void operator()(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<double> &accept_rates) {
    auto &c = comp.contractor;
    // (the reference indexes {row, 2} and {2, col})
    if (c.rows() < 3 || c.cols() < 3) throw std::invalid_argument("MCUpdateSquareTNN3SiteUpdateBase: the lattice needs at least 3 rows and 3 columns");
    auto *self = static_cast<MCUpdater *>(this);
    SweepRowsThenColumns(self, sitps, comp, 3, accept_rates, [&](const SliceSites &s, std::vector<size_t> &acc) {
      c.InitBTen(s.lo(), s.num);
      c.GrowFullBTen(s.hi(), s.num, 3, true);
      const std::vector<TenElemT> psi0 = c.ReplaceTNNSiteTrace(s.at(0), s.dir, 0, {});
      for (size_t w = 0; w < acc.size(); ++w) comp.amplitude[w] = psi0[w] * GradedSign(comp, w);
      for (size_t j = 0; j + 2 < s.N; ++j) {
        const std::vector<uint8_t> a = self->TNN3SiteUpdateImpl(s.at(j), s.at(j + 1), s.at(j + 2), s.dir, sitps, comp);
        for (size_t w = 0; w < acc.size(); ++w) acc[w] += a[w];
        if (j + 3 < s.N) c.ShiftBTenWindow(s.hi());
      }
    });
  }

 protected:
  // the triple table of the component (bosons: of its physical dimension; fermions: TNN3Table of the current mode order), cached
  // under everything it depends on: the states per site, the mode order and the parities of the decoration
  template <typename TenElemT>
  const std::vector<int32_t> &TripleTable(const TPSWaveFunctionComponentT<TenElemT> &comp) {
    std::vector<int> key{(int)comp.contractor.phys_dim(), comp.fermion ? (int)comp.order : -1};
    if (comp.fermion) key.insert(key.end(), comp.fermion->nf.begin(), comp.fermion->nf.end());
    if (key != tab_key_) { tab_ = comp.fermion ? comp.TNN3Table() : TNN3TripleTable(key[0]); tab_key_ = key; }
    return tab_;
  }

 private:
  std::vector<int32_t> tab_;
  std::vector<int> tab_key_;
};

// square_3site_updater.h:98-160
class MCUpdateSquareTNN3SiteExchange : public MCUpdateSquareTNN3SiteUpdateBase<MCUpdateSquareTNN3SiteExchange> {
 public:
  using MCUpdateSquareTNN3SiteUpdateBase<MCUpdateSquareTNN3SiteExchange>::MCUpdateSquareTNN3SiteUpdateBase;
  static constexpr bool kDeviceSliceSweep = true;
  static constexpr bool kDeviceSliceSweepFermions = true;   // (a permutation of three consecutive modes is local in the extended states)
  // one row / column on the device (pepsgpu_sweep_slice_tnn3): walker w consumes the next consumed[w] words of its engine, exactly those
  // TNN3SiteUpdateImpl would draw.  The slice resets the amplitude, so every walker gets its signs back, not only those that moved.
  template <typename TenElemT>
  void SweepSliceOnDevice(BondOrientation dir, size_t slice, const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp,
                          std::vector<size_t> &acc) {
    auto &c = comp.contractor;
    const size_t n = comp.config.walkers(), N = dir == HORIZONTAL ? c.cols() : c.rows(), nwd = 2 * (N - 2);
    const std::vector<uint32_t> words = words_.PeekAll(engines_, nwd);
    std::vector<int32_t> consumed(n), accepted(n), states(n * N);
    std::vector<TenElemT> amp(n);
    check_rc(pepsgpu_sweep_slice_tnn3(c.ctx(), dir, (int)slice, comp.fermion ? TripleTable(comp).data() : nullptr, (int)nwd, words.data(),
                                      dptr(amp.data()), consumed.data(), accepted.data(), states.data()), c.ctx());
    StoreSlice(comp, dir, slice, states, accepted, acc);
    for (size_t w = 0; w < n; ++w) {
      words_.Consume(w, (size_t)consumed[w]);
      comp.amplitude[w] = amp[w] * GradedSign(comp, w);
    }
  }
  // :109-158 batched over the walkers: one ReplaceTNNSiteTrace with the fixed number of candidate slots of the device path (3 for
  // phys_dim 2, else 6), so that both paths run the same kernels on the same operands
  template <typename TenElemT>
  std::vector<uint8_t> TNN3SiteUpdateImpl(const SiteIdx &s1, const SiteIdx &s2, const SiteIdx &s3, BondOrientation dir,
                                          const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp) {
    auto &c = comp.contractor;
    const size_t n = comp.config.walkers();
    const int dp = (int)c.phys_dim(), nslot = dp == 2 ? 3 : 6;
    const std::vector<int32_t> &tab = TripleTable(comp);
    const int32_t d = comp.fermion ? (int32_t)comp.fermion->d() : dp;
    std::vector<int32_t> cand(n * nslot * 3), meta(n * 2);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      int32_t e[3];
      const SiteIdx st[3] = {s1, s2, s3};
      for (int q = 0; q < 3; ++q) e[q] = comp.fermion ? comp.fermion->Ext(comp.config, w, st[q], comp.order) : comp.config(w, st[q]);
      const int32_t *row = tab.data() + ((size_t)(e[0] * dp + e[1]) * dp + e[2]) * kTNN3Tab;
      std::copy(row + 2, row + 2 + 3 * nslot, cand.begin() + (long)(w * nslot * 3));
      meta[2 * w] = row[0];
      meta[2 * w + 1] = row[1];
      any |= row[0] > 1;
    }
    std::vector<uint8_t> changed(n, 0);
    if (!any) return changed;                 // every walker has three equal states (:118)
    const std::vector<TenElemT> alt = c.ReplaceTNNSiteTrace(s1, dir, nslot, cand);
    std::vector<int32_t> ns(n * 3);
    std::vector<TenElemT> new_amp(n);
    for (size_t w = 0; w < n; ++w) {
      const int m = meta[2 * w], init = meta[2 * w + 1];
      if (m <= 1) continue;
      std::vector<TenElemT> psis(m);
      double psi_abs_max = 0;
      for (int i = 0; i < m; ++i) {
        psis[i] = i == init ? comp.amplitude[w] : alt[w * nslot + i];
        psi_abs_max = std::max(psi_abs_max, std::abs(psis[i]));
      }
      std::vector<double> weights(m);
      for (int i = 0; i < m; ++i) weights[i] = std::norm(psis[i] / psi_abs_max);
      QueuedEngine eng = Engine(w);
      const int fin = (int)SuwaTodoStateUpdate((size_t)init, weights, eng);
      if (fin == init) continue;
      changed[w] = 1;
      for (int q = 0; q < 3; ++q) ns[3 * w + q] = cand[(w * nslot + fin) * 3 + q] % d;     // physical states
      new_amp[w] = psis[fin];
    }
    comp.UpdateLocal(new_amp, {s1, s2, s3}, ns, changed);
    return changed;
  }
};

// Result of CalEnergyAndHoles for a walker batch
template <typename TenElemT>
struct EnergyAndHolesT {
  std::vector<TenElemT> energy;                 // [walker]
  std::vector<TenElemT> holes;                  // [walker][row][col][D^4]  (Dag(PunchHole), square_nnn_energy_solver.h:163: the complex conjugate; real: identity)
  std::vector<std::vector<TenElemT>> psi_list;  // [row/col pass][walker]
};
using EnergyAndHoles = EnergyAndHolesT<double>;

// SquareNNNModelEnergySolver (square_nnn_energy_solver.h:37-316) + BondTraversalMixin::TraverseVerticalBonds
// (bond_traversal_mixin.h:113-144).  CRTP hooks:
//   EvaluateBondEnergy(site1, site2, orient, comp, inv_psi) -> [walker]
//   EvaluateNNNEnergy(site1, site2, diagonal_dir, comp, inv_psi) -> [walker]     (has_nnn_interaction only)
//   EvaluateTotalOnsiteEnergy(config, w)
template <class ExplicitlyModel, bool has_nnn_interaction = true>
class SquareNNNModelEnergySolver {
 public:
  template <bool calchols = true, typename TenElemT = double>
  EnergyAndHolesT<TenElemT> CalEnergyAndHoles(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp,
                                              bool holes_on_device = false) {
    const size_t n = comp.config.walkers();
    EnergyAndHolesT<TenElemT> out;
    out.energy.assign(n, TenElemT(0.0));
    auto *self = static_cast<ExplicitlyModel *>(this);
    // The NN bonds of a row / column come from ONE device call for a model whose off-diagonal term exchanges the two site states
    // (kExchangeBondEnergy: real and complex components; fermionic ones for the models with kExchangeBondPsiPerBond) or hops between
    // them (kHopBondEnergy, fermionic components) -- when the holes are not wanted on the host: the slice leaves them in HBM.
    bool dev_slice = false;
    if constexpr (HasExchangeBondEnergy<ExplicitlyModel>::value)
      dev_slice = DeviceSlicesEnabled() && (!comp.fermion || HasExchangeBondPsiPerBond<ExplicitlyModel>::value) && (!calchols || holes_on_device);
    if constexpr (HasHopBondEnergy<ExplicitlyModel>::value)
      dev_slice = DeviceSlicesEnabled() && comp.fermion && (!calchols || holes_on_device);
    out.psi_list = TraverseNNBonds(
        comp, dev_slice, HoleDest<TenElemT>(calchols, holes_on_device, sitps.slot(), comp, out.holes),
        SquareModelBonds<ExplicitlyModel, TenElemT, false, false>(*self, comp),
        [&](const SliceSites &, size_t, const BondValues<TenElemT> &v) {
          for (size_t w = 0; w < n; ++w) out.energy[w] += v.e[w];
        },
        [&](const SliceSites &s, const std::vector<TenElemT> &inv_psi) {
          if constexpr (has_nnn_interaction) {
            bool nnn_slice = false;
            if constexpr (HasExchangeNNNEnergy<ExplicitlyModel>::value) nnn_slice = DeviceSlicesEnabled() && !comp.fermion;
            if (s.dir == HORIZONTAL)
              NNNBondEnergies(*self, comp, nnn_slice, s.num, inv_psi, [&](size_t w, size_t, TenElemT e1, TenElemT e2) { out.energy[w] += e1 + e2; });
          }
        });
    for (size_t w = 0; w < n; ++w) out.energy[w] += self->EvaluateTotalOnsiteEnergy(comp.config, w);   // :99-101
    return out;
  }
};

// square_nn_energy_solver.h:25
template <class ExplicitlyModel>
using SquareNNModelEnergySolver = SquareNNNModelEnergySolver<ExplicitlyModel, false>;

// ---------------------------------------------------------------------------------------------
// Measurement: registry-based observables of a walker batch.
// ObservableMap (model_measurement_solver.h:33-34): key -> flat values; here per walker: values[key][w * len + k].
// Templated over the element type as the reference's ObservableMap<TenElemT>: a complex state has complex local estimators.
template <typename TenElemT>
struct ObservableMapT {
  std::map<std::string, std::vector<TenElemT>> values;
  size_t n = 0;                                               // walkers
  size_t len(const std::string &key) const { return values.at(key).size() / n; }
  std::vector<TenElemT> &make(const std::string &key, size_t length) {
    auto &v = values[key];
    v.assign(n * length, TenElemT(0.0));
    return v;
  }
};
using ObservableMap = ObservableMapT<double>;
struct ObservableMeta {                                        // model_measurement_solver.h:45-63
  std::string key, description;
  std::vector<size_t> shape;
  std::vector<std::string> index_labels;
  std::function<std::string(size_t, size_t)> coord_generator = {};   // (ly, lx) -> the text of stats/<key>_coords.txt, or empty
};
// per walker (model_measurement_solver.h:95-98; PsiConsistencySummary<TenElemT>: psi_mean has the element type, psi_rel_err is real)
template <typename TenElemT>
struct PsiSummaryT { std::vector<TenElemT> psi_mean; std::vector<double> psi_rel_err; };
using PsiSummary = PsiSummaryT<double>;
template <typename TenElemT>
inline std::pair<TenElemT, double> ComputePsiConsistencySummaryAligned(const std::vector<TenElemT> &psi_list);
// what a (non-templated) solver object keeps of its last sample; As<TenElemT>() hands it back in the caller's element type
struct PsiSummaryStore {
  std::vector<std::complex<double>> psi_mean;
  std::vector<double> psi_rel_err;
  // per walker the summary of its amplitudes along the passes of a traversal, psi_list [pass][walker]
  template <typename TenElemT>
  void Fill(size_t n, const std::vector<std::vector<TenElemT>> &psi_list) {
    psi_mean.assign(n, 0.0);
    psi_rel_err.assign(n, 0.0);
    std::vector<TenElemT> one(psi_list.size());
    for (size_t w = 0; w < n; ++w) {
      for (size_t k = 0; k < one.size(); ++k) one[k] = psi_list[k][w];
      const auto s = ComputePsiConsistencySummaryAligned(one);
      psi_mean[w] = s.first;
      psi_rel_err[w] = s.second;
    }
  }
  template <typename TenElemT>
  PsiSummaryT<TenElemT> As() const {
    PsiSummaryT<TenElemT> out;
    out.psi_rel_err = psi_rel_err;
    out.psi_mean.resize(psi_mean.size());
    for (size_t w = 0; w < psi_mean.size(); ++w) {
      if constexpr (ElemTraits<TenElemT>::is_complex) out.psi_mean[w] = psi_mean[w]; else out.psi_mean[w] = psi_mean[w].real();
    }
    return out;
  }
};

// ComputePsiConsistencySummaryAligned (psi_consistency.h:119-168): the largest-magnitude sample is the reference, samples with
// Re[psi_i conj(psi_ref)] < 0 are flipped, (mean, max_i |psi_i - mean| / |mean|)
template <typename TenElemT>
inline std::pair<TenElemT, double> ComputePsiConsistencySummaryAligned(const std::vector<TenElemT> &psi_list) {
  if (psi_list.empty()) return {TenElemT(0.0), 0.0};
  size_t ref = 0;
  for (size_t i = 0; i < psi_list.size(); ++i)
    if (std::abs(psi_list[i]) > std::abs(psi_list[ref])) ref = i;
  const bool ref_valid = std::abs(psi_list[ref]) > 1e-14;
  std::vector<TenElemT> aligned(psi_list);
  TenElemT mean(0.0);
  for (auto &v : aligned) {
    if (ref_valid && std::real(v * ComplexConjugate(psi_list[ref])) < 0.0) v = -v;
    mean += v;
  }
  mean /= (double)aligned.size();
  const double denom = std::max((double)std::abs(mean), std::numeric_limits<double>::epsilon());
  double dev = 0.0;
  for (const TenElemT &v : aligned) dev = std::max(dev, (double)std::abs(v - mean));
  return {mean, dev / denom};
}

// MeasureSpinOneHalfOffDiagOrderInRow (square_spin_onehalf_xxz_obc.h:22-60) for every walker: the valid channel of
// S+(x0) S-(x0+i) / S-(x0) S+(x0+i) along `row`, x0 = lx/4, i = 1..lx/2.  out[w * (lx/2) + i - 1].
template <typename TenElemT>
inline std::vector<TenElemT> MeasureSpinOneHalfOffDiagOrderInRow(TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &inv_psi,
                                                                 size_t row) {
  auto &c = comp.contractor;
  const size_t lx = c.cols(), n = comp.config.walkers(), half = lx / 2;
  const SiteIdx site1{row, lx / 4};
  std::vector<TenElemT> out(n * half, TenElemT(0.0));
  const std::vector<int32_t> sites = {(int32_t)site1.r, (int32_t)site1.c};
  const std::vector<uint8_t> all(n, 1);
  std::vector<int32_t> flipped(n), orig(n);
  for (size_t w = 0; w < n; ++w) { orig[w] = comp.config(w, site1); flipped[w] = 1 - orig[w]; }
  c.UpdateLocal(sites, flipped, all);                 // tn.UpdateSiteTensor(site1, 1 - config(site1)) + EraseEnvsAfterUpdate
  c.CheckInvalidateEnvs(site1);
  c.GrowBTenStep(LEFT);
  c.GrowFullBTen(RIGHT, row, lx / 4 + 2, false);
  for (size_t i = 1; i <= half; ++i) {
    const SiteIdx site2{row, lx / 4 + i};
    std::vector<int32_t> cand(n);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      cand[w] = 1 - comp.config(w, site2);
      any |= comp.config(w, site2) != comp.config(w, site1);
    }
    if (any) {
      std::vector<TenElemT> psi_ex = c.ReplaceOneSiteTrace(site2, HORIZONTAL, 1, cand);
      for (size_t w = 0; w < n; ++w)
        if (comp.config(w, site2) != comp.config(w, site1)) out[w * half + i - 1] = ComplexConjugate(TenElemT(psi_ex[w] * inv_psi[w]));   // :47
    }
    c.ShiftBTenWindow(RIGHT);
  }
  c.UpdateLocal(sites, orig, all);                    // change back (+ EraseEnvsAfterUpdate)
  return out;
}

// SquareNNNModelMeasurementSolver (base/square_nnn_model_measurement_solver.h:23-319) over
// BondTraversalMixin::TraverseAllBonds (base/bond_traversal_mixin.h:22-145).  CRTP hooks of ModelType: the energy-solver
// ones (EvaluateBondEnergy, EvaluateNNNEnergy, EvaluateTotalOnsiteEnergy) plus
//   static constexpr bool requires_spin_sz_measurement / requires_density_measurement, CalSpinSzImpl / CalDensityImpl,
//   EvaluateOffDiagOrderInRow(comp, row, inv_psi, out)   (row hook; may do nothing)
// A fermionic model (kFermionicModel) takes the fermionic traversal below; one with enable_sc_measurement (the t-J family) also
// reports the bond-singlet pairing order through EvaluateBondSC / PairTable / BondSCFromPairs.
template <typename U, typename = void> struct IsFermionicModel : std::false_type {};
template <typename U> struct IsFermionicModel<U, std::void_t<decltype(U::kFermionicModel)>> : std::bool_constant<U::kFermionicModel> {};
template <typename U, typename = void> struct HasSCMeasurement : std::false_type {};
template <typename U> struct HasSCMeasurement<U, std::void_t<decltype(U::enable_sc_measurement)>> : std::bool_constant<U::enable_sc_measurement> {};
// ... and one with the SingletPairCorrelationMixin reports SC_singlet_pair_corr when that is enabled (off by default: nothing changes)
template <typename U, typename = void> struct HasSCPairCorrelation : std::false_type {};
template <typename U>
struct HasSCPairCorrelation<U, std::void_t<decltype(std::declval<const U &>().IsSingletPairCorrelationEnabled())>> : std::true_type {};

template <class ModelType, bool has_nnn_interaction = true>
class SquareNNNModelMeasurementSolver {
 public:
  // The registry of a fermionic model (square_nnn_model_measurement_solver.h:33-215 on a fermionic index; square_tJ_model.h:546-603) over
  // TraverseNNBonds, the traversal of the energy solver.  Per bond the energy hook and, with enable_sc_measurement, the pair estimator:
  //   rho(S') = jw psi(S') / psi(S) = sign ReplaceNNSiteTrace / Trace,  sign = Sigma(S') / Sigma(S) = -1 for a move that changes the
  //   fermion number by +-2 (the decoration leaves Sigma = (-1)^(nf (nf + 1) / 2) out; the column pass's ratio carries jw by itself),
  //   registry value (conj(delta_dag) + delta) / 2 of BondSCFromPairs.
  // Slice path (default): ONE pepsgpu_nn_pair_slice_fermion (kHopBondEnergy: pepsgpu_nn_hop_slice_fermion) per row / column.
  // PEPSHOST_NO_DEVICE_SWEEP=1: the per-bond hooks EvaluateBondEnergy / EvaluateBondSC.  The diagonal bonds (has_nnn_interaction):
  // FermionNNNBondEnergies of the model, zeros where t2 = 0.
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateFermionObservables(TPSWaveFunctionComponentT<TenElemT> &comp) {
    if (!comp.fermion) throw std::logic_error("EvaluateObservables: a fermionic model needs the fermionic decoration of the component");
    auto &c = comp.contractor;
    auto *derived = static_cast<ModelType *>(this);
    const size_t ly = c.rows(), lx = c.cols(), n = comp.config.walkers();
    constexpr bool sc = HasSCMeasurement<ModelType>::value;
    ObservableMapT<TenElemT> out = SiteObservables(comp);
    NNBondMaps<TenElemT> maps(out, ly, lx);
    std::vector<TenElemT> *sc_h = nullptr, *sc_v = nullptr;
    if constexpr (sc) {
      sc_h = &out.make("SC_bond_singlet_h", ly * (lx - 1));
      sc_v = &out.make("SC_bond_singlet_v", (ly - 1) * lx);
    }
    bool use_slice = false;
    if constexpr (HasExchangeBondEnergy<ModelType>::value && HasExchangeBondPsiPerBond<ModelType>::value) use_slice = DeviceSlicesEnabled();
    if constexpr (HasHopBondEnergy<ModelType>::value) use_slice = DeviceSlicesEnabled();
    const std::vector<std::vector<TenElemT>> psi_list = TraverseNNBonds(
        comp, use_slice, HoleDest<TenElemT>(), SquareModelBonds<ModelType, TenElemT, true, sc>(*derived, comp),
        [&](const SliceSites &s, size_t j, const BondValues<TenElemT> &v) {
          maps.Put(s, j, v.e);
          if constexpr (sc)
            for (size_t w = 0; w < n; ++w) (*(s.dir == HORIZONTAL ? sc_h : sc_v))[maps.Index(s, j, w)] = v.sc[w];
        },
        [](const SliceSites &, const std::vector<TenElemT> &) {},
        [&] {
          // SC_singlet_pair_corr inside the row-major phase: its walkers fork from every level of the UP stack and close on every level
          // of the DOWN stack, so the UP stack is grown in full for it and cut back to the vacuum the row pass starts from
          if constexpr (HasSCPairCorrelation<ModelType>::value) {
            if (derived->IsSingletPairCorrelationEnabled()) {
              c.GrowFullBMPS(UP);
              derived->MeasureSingletPairCorrelation(comp, out);
              c.DeleteInnerBMPS(UP);
            }
          }
        });
    // (the same order of additions as the energy solver: bonds, on-site term, diagonal hops)
    auto &en = out.make("energy", 1);
    for (size_t w = 0; w < n; ++w) en[w] = maps.total[w] + derived->EvaluateTotalOnsiteEnergy(comp.config, w);
    if constexpr (has_nnn_interaction) {
      const size_t len_d = (ly - 1) * (lx - 1);
      std::vector<TenElemT> both(n * len_d * 2, TenElemT(0.0));
      derived->FermionNNNBondEnergies(comp, en, &both);
      auto &e_dr = out.make("bond_energy_dr", len_d);
      auto &e_ur = out.make("bond_energy_ur", len_d);
      for (size_t k = 0; k < n * len_d; ++k) { e_dr[k] = both[2 * k]; e_ur[k] = both[2 * k + 1]; }
    }
    last_psi_.Fill(n, psi_list);
    return out;
  }
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp) {
    if constexpr (IsFermionicModel<ModelType>::value) {
      return EvaluateFermionObservables(comp);
    } else {
      return EvaluateBosonObservables(comp);
    }
  }
  // The registry of a bosonic model over the same traversal.  A model of the diagonal-bond traversal with both scalar hooks
  // (BondEnergyFromExchange, NNNEnergyFromExchange) on a bosonic component takes the device slices of the energy solver:
  // pepsgpu_nn_exchange_slice_tab per row / column (no holes) and pepsgpu_nnn_exchange_slice per row pair.
  // MeasureSpinOneHalfOffDiagOrderInRow continues from the BTen stacks the row's bonds leave.  The slice (GrowFullBTen(RIGHT, row, 2)
  // and no shift behind the last bond) ends with LEFT over [0, lx - 2) where the hook loop ends with LEFT over [0, lx - 1), both with the
  // RIGHT stack down to its vacuum; the routine's UpdateLocal at column lx / 4 cuts LEFT back to [0, lx / 4) either way (lx / 4 <=
  // lx - 2 whenever a row has a bond), so it grows the same tensors from the same state.
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateBosonObservables(TPSWaveFunctionComponentT<TenElemT> &comp) {
    auto &c = comp.contractor;
    auto *derived = static_cast<ModelType *>(this);
    const size_t ly = c.rows(), lx = c.cols(), n = comp.config.walkers();
    ObservableMapT<TenElemT> out = SiteObservables(comp);
    NNBondMaps<TenElemT> maps(out, ly, lx);
    std::vector<TenElemT> *e_dr = nullptr, *e_ur = nullptr;
    if constexpr (has_nnn_interaction) {
      e_dr = &out.make("bond_energy_dr", (ly - 1) * (lx - 1));
      e_ur = &out.make("bond_energy_ur", (ly - 1) * (lx - 1));
    }
    bool meas_slice = false;
    if constexpr (has_nnn_interaction && HasExchangeBondEnergy<ModelType>::value && HasExchangeNNNEnergy<ModelType>::value)
      meas_slice = DeviceSlicesEnabled() && !comp.fermion;
    const std::vector<std::vector<TenElemT>> psi_list = TraverseNNBonds(
        comp, meas_slice, HoleDest<TenElemT>(), SquareModelBonds<ModelType, TenElemT, false, false>(*derived, comp),
        [&](const SliceSites &s, size_t j, const BondValues<TenElemT> &v) { maps.Put(s, j, v.e); },
        [&](const SliceSites &s, const std::vector<TenElemT> &inv_psi) {
          if (s.dir != HORIZONTAL) return;
          if constexpr (has_nnn_interaction)
            NNNBondEnergies(*derived, comp, meas_slice, s.num, inv_psi, [&](size_t w, size_t col, TenElemT e1, TenElemT e2) {
              const size_t k = w * (ly - 1) * (lx - 1) + s.num * (lx - 1) + col;
              (*e_dr)[k] = e1; (*e_ur)[k] = e2;
              maps.total[w] += e1 + e2;
            });
          derived->EvaluateOffDiagOrderInRow(comp, s.num, inv_psi, out);
        });
    auto &en = out.make("energy", 1);
    for (size_t w = 0; w < n; ++w) en[w] = maps.total[w] + derived->EvaluateTotalOnsiteEnergy(comp.config, w);
    last_psi_.Fill(n, psi_list);
    return out;
  }
  // psi summary of the sample the last EvaluateObservables call saw (model_measurement_solver.h:101-118, cached path)
  PsiSummary EvaluatePsiSummary() const { return last_psi_.As<double>(); }
  template <typename TenElemT> PsiSummaryT<TenElemT> EvaluatePsiSummaryT() const { return last_psi_.As<TenElemT>(); }
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {   // :256-291
    std::vector<ObservableMeta> out = {{"energy", "Total energy (scalar)", {}, {}}};
    if constexpr (ModelType::requires_spin_sz_measurement) out.push_back({"spin_z", "Local spin Sz per site", {ly, lx}, {"y", "x"}});
    if constexpr (ModelType::requires_density_measurement) out.push_back({"charge", "Local charge per site", {ly, lx}, {"y", "x"}});
    out.push_back({"bond_energy_h", "Bond energy on horizontal NN bonds", {ly, lx > 0 ? lx - 1 : 0}, {"bond_y", "bond_x"}});
    out.push_back({"bond_energy_v", "Bond energy on vertical NN bonds", {ly > 0 ? ly - 1 : 0, lx}, {"bond_y", "bond_x"}});
    if constexpr (has_nnn_interaction) {
      out.push_back({"bond_energy_dr", "Bond energy on diagonal NNN bonds (LeftUp-RightDown)", {ly > 0 ? ly - 1 : 0, lx > 0 ? lx - 1 : 0}, {"bond_y", "bond_x"}});
      out.push_back({"bond_energy_ur", "Bond energy on anti-diagonal NNN bonds (LeftDown-RightUp)", {ly > 0 ? ly - 1 : 0, lx > 0 ? lx - 1 : 0}, {"bond_y", "bond_x"}});
    }
    if constexpr (HasSCMeasurement<ModelType>::value) {      // square_tJ_model.h:657-690
      out.push_back({"SC_bond_singlet_h", "Bond singlet SC (horizontal) avg(conj(delta_dag), delta)", {ly, lx > 0 ? lx - 1 : 0}, {"bond_y", "bond_x"}});
      out.push_back({"SC_bond_singlet_v", "Bond singlet SC (vertical) avg(conj(delta_dag), delta)", {ly > 0 ? ly - 1 : 0, lx}, {"bond_y", "bond_x"}});
    }
    if constexpr (HasSCPairCorrelation<ModelType>::value) static_cast<const ModelType *>(this)->DescribeSingletPairCorrelation(out, ly, lx);
    return out;
  }
 private:
  // a registry with the per-site observables of the configuration: spin_z, charge
  template <typename TenElemT>
  ObservableMapT<TenElemT> SiteObservables(const TPSWaveFunctionComponentT<TenElemT> &comp) {
    auto *derived = static_cast<ModelType *>(this);
    const size_t lx = comp.contractor.cols(), sites = comp.contractor.rows() * lx;
    ObservableMapT<TenElemT> out;
    out.n = comp.config.walkers();
    if constexpr (ModelType::requires_spin_sz_measurement) {
      auto &sz = out.make("spin_z", sites);
      for (size_t w = 0; w < out.n; ++w)
        for (size_t s = 0; s < sites; ++s) sz[w * sites + s] = derived->CalSpinSzImpl(comp.config(w, {s / lx, s % lx}));
    }
    if constexpr (ModelType::requires_density_measurement) {
      auto &ch = out.make("charge", sites);
      for (size_t w = 0; w < out.n; ++w)
        for (size_t s = 0; s < sites; ++s) ch[w * sites + s] = derived->CalDensityImpl(comp.config(w, {s / lx, s % lx}));
    }
    return out;
  }
  // bond_energy_h / _v of a registry and the running total per walker; Index: bond j of a slice -> its place in the h / v arrays
  template <typename TenElemT>
  struct NNBondMaps {
    size_t ly, lx;
    std::vector<TenElemT> &e_h, &e_v, total;
    NNBondMaps(ObservableMapT<TenElemT> &out, size_t ly_, size_t lx_)
        : ly(ly_), lx(lx_), e_h(out.make("bond_energy_h", ly * (lx - 1))), e_v(out.make("bond_energy_v", (ly - 1) * lx)), total(out.n, TenElemT(0.0)) {}
    size_t Index(const SliceSites &s, size_t j, size_t w) const {
      return s.dir == HORIZONTAL ? w * ly * (lx - 1) + s.num * (lx - 1) + j : w * (ly - 1) * lx + j * lx + s.num;
    }
    void Put(const SliceSites &s, size_t j, const std::vector<TenElemT> &e) {
      auto &dst = s.dir == HORIZONTAL ? e_h : e_v;
      for (size_t w = 0; w < e.size(); ++w) { dst[Index(s, j, w)] = e[w]; total[w] += e[w]; }
    }
  };
  PsiSummaryStore last_psi_;
};
template <class ModelType>
using SquareNNModelMeasurementSolver = SquareNNNModelMeasurementSolver<ModelType, false>;

// The spin-1/2 part every XXZ-type model adds on top of the registry traversal (square_spin_onehalf_xxz_obc.h:205-330):
// SzSz_all2all (packed upper triangle, i <= j) and the S+S- / S-S+ channel along the middle row.
struct SpinOneHalfMeasurementHooks {
  static constexpr bool requires_spin_sz_measurement = true;
  static constexpr bool requires_density_measurement = false;
  double CalSpinSzImpl(int32_t config) const { return double(config) - 0.5; }
  double CalDensityImpl(int32_t) const { return 0.0; }
  template <typename TenElemT>
  void EvaluateOffDiagOrderInRow(TPSWaveFunctionComponentT<TenElemT> &comp, size_t row, const std::vector<TenElemT> &inv_psi,
                                 ObservableMapT<TenElemT> &out) const {
    const size_t ly = comp.contractor.rows(), lx = comp.contractor.cols(), n = comp.config.walkers(), half = lx / 2;
    if (row != ly / 2 || half == 0) return;
    std::vector<TenElemT> corr = MeasureSpinOneHalfOffDiagOrderInRow(comp, inv_psi, row);
    auto &smsp = out.make("SmSp_row", half);
    auto &spsm = out.make("SpSm_row", half);
    for (size_t w = 0; w < n; ++w) {
      auto &dst = comp.config(w, {row, lx / 4}) == 0 ? spsm : smsp;      // :279-284
      std::copy(corr.begin() + w * half, corr.begin() + (w + 1) * half, dst.begin() + w * half);
    }
  }
  // StructureFactorMeasurementMixin::MeasureStructureFactor (base/structure_factor_measurement_mixin.h:62-215):
  // SpSm_cross = flat tuples {y1, x1, y2, x2, value} for every y1 < y2; value = amplitude of the configuration with
  // S+ applied at (y1, x1) (source spin down) and S- at (y2, x2) (target spin up), 0 where the channel is closed.
  // As the reference: a main BMPSWalker built on the UP vacuum (:121-122), copied per source site (:134), evolved through the
  // excited row y1 (Evolve with an MPO that is not a row of the network: per-walker states here) and the standard rows below,
  // closed on each row y2 against down_stack[Ly-1-y2] with the walker's own BTen caches (InitBTenLeft to Lx, InitBTenRight at the
  // boundary, scan right to left with TraceWithBTen + GrowBTenRightStep, :160-194).  All Monte-Carlo walkers move in lockstep: a
  // trace is computed for the batch when any walker's channel is open and masked per walker on the host.
  void SetEnableStructureFactor(bool enable) { enable_structure_factor_measurement_ = enable; }
  bool IsStructureFactorEnabled() const { return enable_structure_factor_measurement_; }
  template <typename TenElemT>
  void MeasureStructureFactor(TPSWaveFunctionComponentT<TenElemT> &comp, ObservableMapT<TenElemT> &out) const {
    if (!enable_structure_factor_measurement_) return;
    auto &c = comp.contractor;
    const size_t Ly = c.rows(), Lx = c.cols(), n = comp.config.walkers();
    const size_t per = (Ly - 1) * Lx * Ly / 2 * Lx * 5;       // sum_{y1} Lx * (Ly-1-y1) * Lx tuples of 5
    auto &cross = out.make("SpSm_cross", per);
    std::vector<size_t> fill(n, 0);
    // Default: every DOWN environment is grown first, every pair y1 < y2 is measured.  SetStructureFactorReferenceStackState(true):
    // the mixin exactly as the reference runs it -- it reads GetBMPS(DOWN) as the traversal left it (one level after the row pass),
    // pushes zeros for a row y2 whose environment is not in the stack and `continue`s past the walker's Evolve (:139-149): this
    // form reproduces the reference's regression vector in the oracle (K8, tests/test_oracle_measure.py) and, since round 5, on the
    // device (tests/test_gpu_measure.py::test_k8_reference_structure_factor_regression_on_the_device, 96 values at 1e-10); off by default.
    if (!structure_factor_reference_stack_state_) c.GenerateBMPSApproach(UP);   // UP = vacuum, DOWN fully grown (traversal start state)
    const size_t n_down = c.BMPSStackSize(DOWN);
    auto main_walker = c.MakeWalker(UP, 0);                    // BMPSWalker(tn, up_stack[0], UP, 1, trunc_params)
    const std::vector<int32_t> spin_down(n, 0);                // GetSiteTensor(y2, x2, 0)
    // With the device slices the excited row is built on the device (SetMPOExcited) and the scan of a target row is ONE call with
    // one read-back (TraceSlice: closed walkers skipped inside the contraction, positions closed for every walker not launched);
    // PEPSHOST_NO_DEVICE_SWEEP=1 keeps the per-call body below.
    const bool dev_slice = DeviceSlicesEnabled();
    // S+ at the source: sitps(y1, x1)[1]; S- at the target: component 0 (spin one half: the maps {1, 1} and {0, 0})
    const std::vector<int32_t> to_up(c.phys_dim(), 1), to_down(c.phys_dim(), 0);
    for (size_t y1 = 0; y1 + 1 < Ly; ++y1) {
      for (size_t x1 = 0; x1 < Lx; ++x1) {
        std::vector<uint8_t> src_down(n);
        auto excited_walker = main_walker.Clone();
        if (dev_slice) {
          src_down = excited_walker.SetMPOExcited(y1, x1, to_up);
        } else {
          std::vector<int32_t> excited(n * Lx);
          for (size_t w = 0; w < n; ++w) {
            for (size_t x = 0; x < Lx; ++x) excited[w * Lx + x] = comp.config(w, {y1, x});
            src_down[w] = comp.config(w, {y1, x1}) == 0;
            if (src_down[w]) excited[w * Lx + x1] = 1;          // excited_mpo_ptrs[x1] = sitps(y1, x1)[1]
          }
          excited_walker.SetMPOStates(y1, excited);
        }
        excited_walker.Evolve();                                // absorb the excited row y1
        for (size_t y2 = y1 + 1; y2 < Ly; ++y2) {
          const size_t bottom = Ly - 1 - y2;                    // bottom_env = down_stack[Ly-1-y2]
          if (bottom >= n_down) {                               // (:139-149; only in the reference stack state)
            for (size_t w = 0; w < n; ++w)
              for (size_t x2 = 0; x2 < Lx; ++x2) {
                TenElemT *t = &cross[w * per + fill[w]];
                t[0] = (double)y1; t[1] = (double)x1; t[2] = (double)y2; t[3] = (double)x2; t[4] = 0.0;
                fill[w] += 5;
              }
            continue;
          }
          excited_walker.SetMPO(y2);                            // standard_mpo = tn.get_row(y2)
          std::vector<TenElemT> row;
          if (dev_slice) {
            row = excited_walker.TraceSlice(bottom, to_down, src_down);
          } else {
            excited_walker.InitBTenLeft(bottom, Lx);
            excited_walker.InitBTenRight(bottom, Lx - 1);
            row.assign(n * Lx, TenElemT(0.0));
            for (size_t x2r = 0; x2r < Lx; ++x2r) {
              const size_t x2 = Lx - 1 - x2r;
              bool any = false;
              for (size_t w = 0; w < n; ++w) any |= src_down[w] && comp.config(w, {y2, x2}) == 1;
              if (any) {
                std::vector<TenElemT> psi_ex = excited_walker.TraceWithBTen(bottom, x2, spin_down);
                for (size_t w = 0; w < n; ++w)
                  if (src_down[w] && comp.config(w, {y2, x2}) == 1) row[w * Lx + x2] = psi_ex[w];
              }
              if (x2 > 0) excited_walker.GrowBTenRightStep(bottom);
            }
          }
          for (size_t w = 0; w < n; ++w)
            for (size_t x2 = 0; x2 < Lx; ++x2) {
              TenElemT *t = &cross[w * per + fill[w]];
              t[0] = (double)y1; t[1] = (double)x1; t[2] = (double)y2; t[3] = (double)x2; t[4] = row[w * Lx + x2];
              fill[w] += 5;
            }
          excited_walker.ClearBTen();
          if (y2 + 1 < Ly) excited_walker.Evolve();             // absorb row y2 with the standard MPO
        }
      }
      main_walker.SetMPO(y1);
      main_walker.Evolve();                                     // main_walker.Evolve(standard row y1)
    }
  }
  bool enable_structure_factor_measurement_ = false;
  void SetStructureFactorReferenceStackState(bool on) { structure_factor_reference_stack_state_ = on; }
  bool structure_factor_reference_stack_state_ = false;

  template <typename TenElemT>
  static void AddSzSzAll2All(const TPSWaveFunctionComponentT<TenElemT> &comp, ObservableMapT<TenElemT> &out) {   // :225-236
    const size_t ly = comp.contractor.rows(), lx = comp.contractor.cols(), n = comp.config.walkers(), N = ly * lx;
    auto &szsz = out.make("SzSz_all2all", N * (N + 1) / 2);
    for (size_t w = 0; w < n; ++w) {
      size_t k = w * (N * (N + 1) / 2);
      for (size_t i = 0; i < N; ++i) {
        const double szi = double(comp.config(w, {i / lx, i % lx})) - 0.5;
        for (size_t j = i; j < N; ++j) szsz[k++] = szi * (double(comp.config(w, {j / lx, j % lx})) - 0.5);
      }
    }
  }
  static void DescribeSpinOneHalf(std::vector<ObservableMeta> &base, size_t ly, size_t lx) {   // :296-330
    const size_t N = ly * lx;
    base.push_back({"SzSz_all2all", "Packed upper-triangular SzSz(i,j) with i<=j (flat)", {N * (N + 1) / 2}, {"pair_packed_upper_tri"}});
    base.push_back({"SmSp_row", "Row Sm(i)Sp(j) along middle row (flat)", {lx / 2}, {"segment"}});
    base.push_back({"SpSm_row", "Row Sp(i)Sm(j) along middle row (flat)", {lx / 2}, {"segment"}});
  }
};

// SquareSpinOneHalfXXZModelMixIn (square_spin_onehalf_xxz_obc.h:64-141): the bond / NNN-link / on-site terms
class SquareSpinOneHalfXXZModelMixIn {
 public:
  SquareSpinOneHalfXXZModelMixIn(double jz, double jxy, double jz2, double jxy2, double pinning00)
      : jz_(jz), jxy_(jxy), jz2_(jz2), jxy2_(jxy2), pinning00_(pinning00) {}
  template <typename TenElemT>
  std::vector<TenElemT> EvaluateBondEnergy(const SiteIdx &s1, const SiteIdx &s2, BondOrientation orient,
                                           TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &inv_psi) {   // :72-104
    const size_t n = comp.config.walkers();
    std::vector<int32_t> cand(n * 2);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      cand[2 * w] = comp.config(w, s2);
      cand[2 * w + 1] = comp.config(w, s1);
      any |= cand[2 * w] != cand[2 * w + 1];
    }
    std::vector<TenElemT> e(n, TenElemT(0.25 * jz_));
    if (!any) return e;
    std::vector<TenElemT> psi_ex = comp.ReplaceNNSiteTrace(s1, s2, orient, 1, cand);
    for (size_t w = 0; w < n; ++w)
      if (comp.config(w, s1) != comp.config(w, s2)) e[w] = -0.25 * jz_ + ComplexConjugate(TenElemT(psi_ex[w] * inv_psi[w])) * (0.5 * jxy_);   // :98-100
    return e;
  }
  // :107-134; site1 = left end of the diagonal, site2 = right end
  template <typename TenElemT>
  std::vector<TenElemT> EvaluateNNNEnergy(const SiteIdx &s1, const SiteIdx &s2, DIAGONAL_DIR diagonal_dir,
                                          TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &inv_psi) {
    const size_t n = comp.config.walkers();
    std::vector<int32_t> cand(n * 2);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      cand[2 * w] = comp.config(w, s2);
      cand[2 * w + 1] = comp.config(w, s1);
      any |= cand[2 * w] != cand[2 * w + 1];
    }
    std::vector<TenElemT> e(n, TenElemT(0.25 * jz2_));
    if (!any) return e;
    const SiteIdx left_up = diagonal_dir == LEFTUP_TO_RIGHTDOWN ? s1 : SiteIdx{s2.r, s1.c};
    std::vector<TenElemT> psi_ex = comp.contractor.ReplaceNNNSiteTrace(left_up, diagonal_dir, HORIZONTAL, 1, cand);
    for (size_t w = 0; w < n; ++w)
      if (comp.config(w, s1) != comp.config(w, s2)) e[w] = -0.25 * jz2_ + ComplexConjugate(TenElemT(psi_ex[w] * inv_psi[w])) * (0.5 * jxy2_);
    return e;
  }
  double EvaluateTotalOnsiteEnergy(const Configuration &config, size_t w) const {   // :139-141
    return -pinning00_ * (double(config(w, {0, 0})) - 0.5);
  }
  // the bond term as a function of the two states and psi(exchanged) / psi (:98-100): what EvaluateBondEnergy computes per walker
  static constexpr bool kExchangeBondEnergy = true;
  template <typename TenElemT>
  TenElemT BondEnergyFromExchange(int32_t config1, int32_t config2, TenElemT ratio) const {
    return config1 == config2 ? TenElemT(0.25 * jz_) : TenElemT(-0.25 * jz_ + ratio * (0.5 * jxy_));
  }
  // the diagonal-link term likewise (:107-134): what EvaluateNNNEnergy computes per walker
  static constexpr bool kExchangeNNNEnergy = true;
  template <typename TenElemT>
  TenElemT NNNEnergyFromExchange(int32_t config1, int32_t config2, TenElemT ratio) const {
    return config1 == config2 ? TenElemT(0.25 * jz2_) : TenElemT(-0.25 * jz2_ + ratio * (0.5 * jxy2_));
  }
 protected:
  double jz_, jxy_, jz2_, jxy2_, pinning00_;
};

// square_spin_onehalf_xxz_obc.h:174-190
class SquareSpinOneHalfXXZModelOBC : public SquareNNModelEnergySolver<SquareSpinOneHalfXXZModelOBC>,
                                     public SquareNNModelMeasurementSolver<SquareSpinOneHalfXXZModelOBC>,
                                     public SpinOneHalfMeasurementHooks,
                                     public SquareSpinOneHalfXXZModelMixIn {
 public:
  SquareSpinOneHalfXXZModelOBC() : SquareSpinOneHalfXXZModelMixIn(1.0, 1.0, 0.0, 0.0, 0.0) {}
  SquareSpinOneHalfXXZModelOBC(double jz, double jxy, double pinning00)
      : SquareSpinOneHalfXXZModelMixIn(jz, jxy, 0.0, 0.0, pinning00) {}
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp) {   // :215-251
    ObservableMapT<TenElemT> out = SquareNNModelMeasurementSolver<SquareSpinOneHalfXXZModelOBC>::EvaluateObservables(sitps, comp);
    AddSzSzAll2All(comp, out);
    MeasureStructureFactor(comp, out);                         // :238-248 (if enabled)
    return out;
  }
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {
    auto base = SquareNNModelMeasurementSolver<SquareSpinOneHalfXXZModelOBC>::DescribeObservables(ly, lx);
    DescribeSpinOneHalf(base, ly, lx);
    return base;
  }
};

// square_spin_onehalf_j1j2_xxz_obc.h:25-40
class SquareSpinOneHalfJ1J2XXZModelOBC : public SquareNNNModelEnergySolver<SquareSpinOneHalfJ1J2XXZModelOBC>,
                                         public SquareNNNModelMeasurementSolver<SquareSpinOneHalfJ1J2XXZModelOBC>,
                                         public SpinOneHalfMeasurementHooks,
                                         public SquareSpinOneHalfXXZModelMixIn {
 public:
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp) {
    ObservableMapT<TenElemT> out = SquareNNNModelMeasurementSolver<SquareSpinOneHalfJ1J2XXZModelOBC>::EvaluateObservables(sitps, comp);
    AddSzSzAll2All(comp, out);
    return out;
  }
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {
    auto base = SquareNNNModelMeasurementSolver<SquareSpinOneHalfJ1J2XXZModelOBC>::DescribeObservables(ly, lx);
    DescribeSpinOneHalf(base, ly, lx);
    return base;
  }
  explicit SquareSpinOneHalfJ1J2XXZModelOBC(double j2) : SquareSpinOneHalfXXZModelMixIn(1, 1, j2, j2, 0) {}
  SquareSpinOneHalfJ1J2XXZModelOBC(double jz, double jxy, double jz2, double jxy2, double pinning_field00)
      : SquareSpinOneHalfXXZModelMixIn(jz, jxy, jz2, jxy2, pinning_field00) {}
};

// spin_onehalf_triangle_heisenberg_sqrpeps.h:39-229: the spin-1/2 Heisenberg model of the TRIANGULAR lattice on a square PEPS -- the
// nearest-neighbour bonds of the square lattice plus ONE diagonal of every plaquette (left-down to right-up), all with J = 1
// (EvaluateBondEnergy :66-85, EvaluateNNNEnergy :87-112: zero for the other diagonal).  Registry: the generic NNN traversal minus
// `bond_energy_dr` (:126-127), SzSz_all2all, the row channels (hooks of the XXZ model), the structure factor behind its switch.
class SpinOneHalfTriHeisenbergSqrPEPS : public SquareNNNModelEnergySolver<SpinOneHalfTriHeisenbergSqrPEPS>,
                                        public SquareNNNModelMeasurementSolver<SpinOneHalfTriHeisenbergSqrPEPS>,
                                        public SpinOneHalfMeasurementHooks,
                                        public SquareSpinOneHalfXXZModelMixIn {
 public:
  SpinOneHalfTriHeisenbergSqrPEPS() : SquareSpinOneHalfXXZModelMixIn(1, 1, 1, 1, 0) {}
  static constexpr int kNNNDiagMask = 2;              // only LEFTDOWN_TO_RIGHTUP interacts (:98-100): the other diagonal is exactly 0
  template <typename TenElemT>
  std::vector<TenElemT> EvaluateNNNEnergy(const SiteIdx &s1, const SiteIdx &s2, DIAGONAL_DIR diagonal_dir,
                                          TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &inv_psi) {
    if (diagonal_dir != LEFTDOWN_TO_RIGHTUP) return std::vector<TenElemT>(comp.config.walkers(), TenElemT(0));   // :98-100
    return SquareSpinOneHalfXXZModelMixIn::EvaluateNNNEnergy(s1, s2, diagonal_dir, comp, inv_psi);
  }
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp) {
    ObservableMapT<TenElemT> out = SquareNNNModelMeasurementSolver<SpinOneHalfTriHeisenbergSqrPEPS>::EvaluateObservables(sitps, comp);
    out.values.erase("bond_energy_dr");               // "legacy public API: only the interacting diagonal" (:126-127)
    AddSzSzAll2All(comp, out);
    return out;
  }
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {
    auto base = SquareNNNModelMeasurementSolver<SpinOneHalfTriHeisenbergSqrPEPS>::DescribeObservables(ly, lx);
    base.erase(std::remove_if(base.begin(), base.end(), [](const ObservableMeta &m) { return m.key == "bond_energy_dr"; }), base.end());
    DescribeSpinOneHalf(base, ly, lx);
    return base;
  }
};

// spin_onehalf_triangle_heisenbergJ1J2_sqrpeps.h:48-463: the J1-J2 Heisenberg model of the triangular lattice on a square PEPS.
// J1 = 1 on the horizontal and vertical bonds and on the left-down -> right-up diagonal of every plaquette; J2 on the three links of
// distance sqrt 3: the other plaquette diagonal (r, c)-(r+1, c+1), the flat sqrt5 link (r+1, c)-(r, c+2) of a 2 x 3 window and the steep
// sqrt5 link (r+2, c)-(r, c+1) of a 3 x 2 window.  The model has its own traversal (CalEnergyAndHolesImpl :304-446): the row pass
// carries the horizontal bonds on BTen and both diagonals + the flat link on BTen2, the column pass the vertical bonds on BTen and the
// steep link on BTen2 (GrowFullBTen2(DOWN, col, 3)); with the device slices each row, column, row pair and column pair is ONE device
// call (pepsgpu_nn_exchange_slice_tab, pepsgpu_link_exchange_slice).  Registry (:65-277): energy, spin_z, bond_energy_h / v / ur (the J2 links only
// enter the energy scalar), SzSz_row / SmSp_row / SpSm_row of the middle row, SzSz_all2all (+-0.25, :449-463).
class SpinOneHalfTriJ1J2HeisenbergSqrPEPS : public SpinOneHalfMeasurementHooks {
 public:
  explicit SpinOneHalfTriJ1J2HeisenbergSqrPEPS(double j2) : j2_(j2) {}
  enum BondKind { BOND_H, BOND_V, BOND_UR, BOND_DR, BOND_FLAT, BOND_STEEP };

  template <bool calchols = true, typename TenElemT = double>
  EnergyAndHolesT<TenElemT> CalEnergyAndHoles(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp,
                                              bool holes_on_device = false) {
    const size_t n = comp.config.walkers();
    EnergyAndHolesT<TenElemT> out;
    std::vector<TenElemT> e1(n, TenElemT(0.0)), e2(n, TenElemT(0.0));
    Traverse<TenElemT>(sitps, comp, calchols, holes_on_device, out, [&](BondKind kind, const SiteIdx &, const SiteIdx &, const std::vector<TenElemT> &e) {
      auto &dst = kind <= BOND_UR ? e1 : e2;
      for (size_t w = 0; w < n; ++w) dst[w] += e[w];
    });
    out.energy.resize(n);
    for (size_t w = 0; w < n; ++w) out.energy[w] = e1[w] + j2_ * e2[w];       // :445
    return out;
  }

  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp) {
    auto &c = comp.contractor;
    const size_t ly = c.rows(), lx = c.cols(), n = comp.config.walkers(), half = lx / 2;
    ObservableMapT<TenElemT> out;
    out.n = n;
    auto &sz = out.make("spin_z", ly * lx);
    for (size_t w = 0; w < n; ++w)
      for (size_t r = 0; r < ly; ++r)
        for (size_t cc = 0; cc < lx; ++cc) sz[w * ly * lx + r * lx + cc] = double(comp.config(w, {r, cc})) - 0.5;
    auto &e_h = out.make("bond_energy_h", ly * (lx - 1));
    auto &e_v = out.make("bond_energy_v", (ly - 1) * lx);
    auto &e_ur = out.make("bond_energy_ur", (ly - 1) * (lx - 1));
    std::vector<TenElemT> e1(n, TenElemT(0.0)), e2(n, TenElemT(0.0));
    EnergyAndHolesT<TenElemT> scratch;
    Traverse<TenElemT>(sitps, comp, false, false, scratch, [&](BondKind kind, const SiteIdx &s1, const SiteIdx &s2, const std::vector<TenElemT> &e) {
      for (size_t w = 0; w < n; ++w) {
        if (kind == BOND_H) e_h[w * ly * (lx - 1) + s1.r * (lx - 1) + s1.c] = e[w];
        else if (kind == BOND_V) e_v[w * (ly - 1) * lx + s1.r * lx + s1.c] = e[w];
        else if (kind == BOND_UR) e_ur[w * (ly - 1) * (lx - 1) + s2.r * (lx - 1) + s1.c] = e[w];       // e_ur(row, col): top-left cell (:201)
        (kind <= BOND_UR ? e1 : e2)[w] += e[w];
      }
    });
    auto &en = out.make("energy", 1);
    for (size_t w = 0; w < n; ++w) en[w] = e1[w] + j2_ * e2[w];
    // middle row (:131-171): SzSz along the row, then the S+S- / S-S+ channel.  The traversal has left the stacks in the column pass:
    // the row window is rebuilt (the reference runs this block inside the row pass; same environments, same numbers).
    const size_t row = ly / 2;
    if (half > 0) {
      auto &szsz = out.make("SzSz_row", half);
      for (size_t w = 0; w < n; ++w) {
        const double sz1 = double(comp.config(w, {row, lx / 4})) - 0.5;
        for (size_t i = 1; i <= half; ++i) szsz[w * half + i - 1] = sz1 * (double(comp.config(w, {row, lx / 4 + i})) - 0.5);
      }
      comp.SetOrder(ROW_MAJOR);
      c.GenerateBMPSApproach(UP);
      for (size_t r = 0; r < row; ++r) c.ShiftBMPSWindow(DOWN);
      c.InitBTen(LEFT, row);
      c.GrowFullBTen(RIGHT, row, 1, true);
      std::vector<TenElemT> inv_psi = c.Trace({row, 0}, HORIZONTAL);
      for (auto &v : inv_psi) v = TenElemT(1.0) / v;
      for (size_t col = 0; col + 1 < lx; ++col) c.ShiftBTenWindow(RIGHT);
      EvaluateOffDiagOrderInRow(comp, row, inv_psi, out);
    }
    const size_t N = ly * lx;                                                   // :260-275, :449-463
    auto &all = out.make("SzSz_all2all", N * (N + 1) / 2);
    for (size_t w = 0; w < n; ++w) {
      size_t k = w * (N * (N + 1) / 2);
      for (size_t i = 0; i < N; ++i)
        for (size_t j = i; j < N; ++j)
          all[k++] = comp.config(w, {i / lx, i % lx}) == comp.config(w, {j / lx, j % lx}) ? 0.25 : -0.25;
    }
    last_psi_.Fill(n, scratch.psi_list);
    return out;
  }
  PsiSummary EvaluatePsiSummary() const { return last_psi_.As<double>(); }
  template <typename TenElemT> PsiSummaryT<TenElemT> EvaluatePsiSummaryT() const { return last_psi_.As<TenElemT>(); }
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {   // :279-297
    const size_t N = ly * lx;
    return {{"energy", "Total energy (scalar)", {}, {}},
            {"spin_z", "Local spin Sz per site (Ly,Lx)", {ly, lx}, {"y", "x"}},
            {"SzSz_row", "Row SzSz correlations along middle row (flat)", {lx / 2}, {"segment"}},
            {"SmSp_row", "Row Sm(i)Sp(j) along middle row (flat)", {lx / 2}, {"segment"}},
            {"SpSm_row", "Row Sp(i)Sm(j) along middle row (flat)", {lx / 2}, {"segment"}},
            {"bond_energy_h", "Bond energy on horizontal NN bonds (flat)", {ly * (lx > 0 ? lx - 1 : 0)}, {"bond"}},
            {"bond_energy_v", "Bond energy on vertical NN bonds (flat)", {(ly > 0 ? ly - 1 : 0) * lx}, {"bond"}},
            {"bond_energy_ur", "Bond energy on diagonal (triangular, Up-Right) bonds (flat)", {(ly > 0 ? ly - 1 : 0) * (lx > 0 ? lx - 1 : 0)}, {"bond"}},
            {"SzSz_all2all", "All-to-all SzSz correlations (upper-tri packed)", {N * (N + 1) / 2}, {"pair_packed_upper_tri"}}};
  }

 private:
  // 0.25 for equal spins, else -0.25 + 0.5 conj(psi_ex / psi) (:338-345 and the seven other bond blocks); trace(cand) is only called
  // when some walker's two spins differ.
  template <typename TenElemT, class TraceFn>
  static std::vector<TenElemT> Bond(const TPSWaveFunctionComponentT<TenElemT> &comp, const SiteIdx &s1, const SiteIdx &s2,
                                    const std::vector<TenElemT> &inv_psi, TraceFn trace) {
    const size_t n = comp.config.walkers();
    std::vector<int32_t> cand(n * 2);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      cand[2 * w] = comp.config(w, s2);
      cand[2 * w + 1] = comp.config(w, s1);
      any |= cand[2 * w] != cand[2 * w + 1];
    }
    std::vector<TenElemT> e(n, TenElemT(0.25));
    if (!any) return e;
    std::vector<TenElemT> psi_ex = trace(cand);
    for (size_t w = 0; w < n; ++w)
      if (comp.config(w, s1) != comp.config(w, s2)) e[w] = -0.25 + ComplexConjugate(TenElemT(psi_ex[w] * inv_psi[w])) * 0.5;
    return e;
  }
  // ... with psi_ex = value(w) from a slice's table
  template <typename TenElemT, class Value>
  static std::vector<TenElemT> SliceBond(const TPSWaveFunctionComponentT<TenElemT> &comp, const SiteIdx &s1, const SiteIdx &s2,
                                         const std::vector<TenElemT> &inv_psi, Value value) {
    std::vector<TenElemT> e(inv_psi.size(), TenElemT(0.25));
    for (size_t w = 0; w < e.size(); ++w)
      if (comp.config(w, s1) != comp.config(w, s2)) e[w] = -0.25 + ComplexConjugate(TenElemT(value(w) * inv_psi[w])) * 0.5;
    return e;
  }
  // the h / v bonds for TraverseNNBonds: the exchange slice, or a ReplaceNNSiteTrace per bond
  template <typename TenElemT>
  struct NNBonds {
    TPSWaveFunctionComponentT<TenElemT> &comp;
    BondSlice<TenElemT> Read(const SliceSites &s, bool holes) const { return ExchangeSlice(comp, s, holes, false); }
    std::vector<TenElemT> FromSlice(const SliceSites &s, size_t j, const BondSlice<TenElemT> &sl, const std::vector<TenElemT> &inv_psi) const {
      return SliceBond(comp, s.at(j), s.at(j + 1), inv_psi, [&](size_t w) { return sl.ex[w * sl.np + j]; });
    }
    std::vector<TenElemT> Hook(const SliceSites &s, size_t j, const std::vector<TenElemT> &inv_psi) const {
      const SiteIdx s1 = s.at(j), s2 = s.at(j + 1);
      return Bond<TenElemT>(comp, s1, s2, inv_psi, [&](const std::vector<int32_t> &cand) { return comp.ReplaceNNSiteTrace(s1, s2, s.dir, 1, cand); });   // :338-345
    }
  };
  // on_bond(kind, site1, site2, e [walker]) for every bond and link in the order of CalEnergyAndHolesImpl (:304-446); the holes and the
  // psi list into out.  The h / v bonds are those of TraverseNNBonds (under the device-slice condition of SquareNNNModelEnergySolver:
  // no holes, or holes resident on the device); the links of a row pair / column pair hang behind the row / column: ONE
  // pepsgpu_link_exchange_slice each with the device slices (bosonic component; they do not depend on where the holes go), else a
  // trace per link over the BTen2 of the pair.
  template <typename TenElemT, class OnBond>
  void Traverse(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp, bool calchols, bool holes_on_device,
                EnergyAndHolesT<TenElemT> &out, OnBond on_bond) {
    auto &c = comp.contractor;
    const size_t rows = c.rows(), cols = c.cols(), n = comp.config.walkers();
    const bool link_slice = DeviceSlicesEnabled() && !comp.fermion;
    const bool nn_slice = link_slice && (!calchols || holes_on_device);
    // the link table [n][N - 1][4] of a row pair / column pair
    auto links = [&](BondOrientation dir, size_t slice, int mask) {
      std::vector<TenElemT> val(n * ((dir == HORIZONTAL ? cols : rows) - 1) * 4);
      check_rc(pepsgpu_link_exchange_slice(c.ctx(), dir, (int)slice, mask, dptr(val.data())), c.ctx());
      return val;
    };
    auto row_links = [&](size_t row, const std::vector<TenElemT> &inv_psi) {
      if (row + 1 >= rows) return;
      if (link_slice) {
        const std::vector<TenElemT> val = links(HORIZONTAL, row, 1 | 2 | 8);   // both diagonals and the flat link (r+1, c)-(r, c+2)
        for (size_t col = 0; col + 1 < cols; col++) {
          auto kind = [&val, col, np = cols - 1](int k) { return [&val, col, k, np](size_t w) { return val[(w * np + col) * 4 + k]; }; };
          on_bond(BOND_UR, {row + 1, col}, {row, col + 1}, SliceBond(comp, {row + 1, col}, {row, col + 1}, inv_psi, kind(1)));
          on_bond(BOND_DR, {row, col}, {row + 1, col + 1}, SliceBond(comp, {row, col}, {row + 1, col + 1}, inv_psi, kind(0)));
          if (col + 2 < cols) on_bond(BOND_FLAT, {row + 1, col}, {row, col + 2}, SliceBond(comp, {row + 1, col}, {row, col + 2}, inv_psi, kind(3)));
        }
        return;
      }
      c.InitBTen2(LEFT, row);                                                // :350
      c.GrowFullBTen2(RIGHT, row, 2, true);
      for (size_t col = 0; col + 1 < cols; col++) {
        const SiteIdx lu{row, col};
        {
          const SiteIdx s1{row + 1, col}, s2{row, col + 1};                  // :355-367 J1 diagonal
          on_bond(BOND_UR, s1, s2, Bond<TenElemT>(comp, s1, s2, inv_psi, [&](const std::vector<int32_t> &cand) {
                    return c.ReplaceNNNSiteTrace(lu, LEFTDOWN_TO_RIGHTUP, HORIZONTAL, 1, cand); }));
        }
        {
          const SiteIdx s1{row, col}, s2{row + 1, col + 1};                  // :369-381 J2 diagonal
          on_bond(BOND_DR, s1, s2, Bond<TenElemT>(comp, s1, s2, inv_psi, [&](const std::vector<int32_t> &cand) {
                    return c.ReplaceNNNSiteTrace(lu, LEFTUP_TO_RIGHTDOWN, HORIZONTAL, 1, cand); }));
        }
        if (col + 2 < cols) {                                                // :383-397 flat sqrt5 link
          const SiteIdx s1{row + 1, col}, s2{row, col + 2};
          on_bond(BOND_FLAT, s1, s2, Bond<TenElemT>(comp, s1, s2, inv_psi, [&](const std::vector<int32_t> &cand) {
                    return c.ReplaceSqrt5DistTwoSiteTrace(lu, LEFTDOWN_TO_RIGHTUP, HORIZONTAL, 1, cand); }));
        }
        c.ShiftBTen2Window(RIGHT, row);                                      // :398
      }
    };
    auto column_links = [&](size_t col, const std::vector<TenElemT> &inv_psi) {
      if (col + 1 >= cols) return;
      if (link_slice && rows >= 3) {
        const std::vector<TenElemT> val = links(VERTICAL, col, 8);            // the steep link (r+2, c)-(r, c+1)
        for (size_t row = 0; row + 2 < rows; row++)
          on_bond(BOND_STEEP, {row + 2, col}, {row, col + 1}, SliceBond(comp, {row + 2, col}, {row, col + 1}, inv_psi,
                  [&](size_t w) { return val[(w * (rows - 1) + row) * 4 + 3]; }));
        return;
      }
      c.InitBTen2(UP, col);                                                  // :425
      c.GrowFullBTen2(DOWN, col, 3, true);
      for (size_t row = 0; row + 2 < rows; row++) {                          // :428-442 steep sqrt5 link
        const SiteIdx s1{row + 2, col}, s2{row, col + 1};
        on_bond(BOND_STEEP, s1, s2, Bond<TenElemT>(comp, s1, s2, inv_psi, [&](const std::vector<int32_t> &cand) {
                  return c.ReplaceSqrt5DistTwoSiteTrace({row, col}, LEFTDOWN_TO_RIGHTUP, VERTICAL, 1, cand); }));
        if (row + 3 < rows) c.ShiftBTen2Window(DOWN, col);
      }
    };
    out.psi_list = TraverseNNBonds(
        comp, nn_slice, HoleDest<TenElemT>(calchols, holes_on_device, sitps.slot(), comp, out.holes), NNBonds<TenElemT>{comp},
        [&](const SliceSites &s, size_t j, const std::vector<TenElemT> &e) { on_bond(s.dir == HORIZONTAL ? BOND_H : BOND_V, s.at(j), s.at(j + 1), e); },
        [&](const SliceSites &s, const std::vector<TenElemT> &inv_psi) {
          if (s.dir == HORIZONTAL) row_links(s.num, inv_psi); else column_links(s.num, inv_psi);
        });
  }
  double j2_;
  PsiSummaryStore last_psi_;
};

// The diagonal (next-nearest-neighbour) hop of the fermionic models, -t2 sum_<<ij>> (c+_i c_j + h.c.): square_spinless_fermion.h:161-200
// and square_tJ_model.h:424-463.  E_loc += -t2 jw ComplexConjugate(psi(S') / psi(S)) per diagonal with exactly one end occupied
// (spinless: occupied <-> empty; t-J: an electron moves into a hole, two spins never exchange), S' = S with the two end states
// exchanged, jw = (-1)^(fermions strictly between the two ends in row-major order).  Three paths:
//   Slice  one pepsgpu_nnn_hop_slice_fermion call per row pair (the default wherever DeviceSlicesEnabled());
//   Local  the same contractions driven per plaquette from the host (PEPSHOST_NO_DEVICE_SWEEP=1);
//   Fresh  one fresh batched contraction per diagonal (PEPSHOST_NNN_FRESH=1; the independent check).
struct FermionNNNHop {
  // bonds (optional, zero-filled by the caller): [walker][rows - 1][cols - 1][2] receives the term of every diagonal, entry 0
  // LEFTUP_TO_RIGHTDOWN, entry 1 LEFTDOWN_TO_RIGHTUP (the measurement registry's bond_energy_dr / _ur)
  template <typename TenElemT>
  static void Add(double t2, TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds = nullptr) {
    static const bool fresh = getenv("PEPSHOST_NNN_FRESH") != nullptr;
    if (t2 == 0.0) return;
    if (fresh) Fresh(t2, comp, energy, bonds);
    else if (DeviceSlicesEnabled()) Slice(t2, comp, energy, bonds);
    else Local(t2, comp, energy, bonds);
  }
  template <typename TenElemT>
  static void Put(std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds, size_t w, size_t rows, size_t cols, size_t row, size_t col,
                  int diag, TenElemT e) {
    energy[w] += e;
    if (bonds) (*bonds)[((w * (rows - 1) + row) * (cols - 1) + col) * 2 + diag] = e;
  }
  template <typename TenElemT>
  static void Slice(double t2, TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds = nullptr) {
    if (!comp.fermion) throw std::logic_error("fermionic NNN hopping needs the fermionic decoration of the component");
    const size_t n = comp.config.walkers(), rows = comp.config.rows(), cols = comp.config.cols();
    if (rows < 2 || cols < 2) return;
    const FermionDecoration &fd = *comp.fermion;
    auto &ct = comp.contractor;
    comp.SetOrder(ROW_MAJOR);
    comp.InitDevice();
    std::vector<int32_t> occ(fd.d());
    for (size_t s = 0; s < occ.size(); ++s) occ[s] = fd.n((int32_t)s);
    const size_t np = cols - 1;
    std::vector<TenElemT> psi(n * np), val(n * np * 2);
    ct.GenerateBMPSApproach(UP);
    for (size_t row = 0; row + 1 < rows; ++row) {
      check_rc(pepsgpu_nnn_hop_slice_fermion(ct.ctx(), (int)row, (int)fd.d(), occ.data(), 3, dptr(psi.data()), dptr(val.data())), ct.ctx());
      for (size_t w = 0; w < n; ++w)
        for (size_t col = 0; col < np; ++col) {
          const SiteIdx q[4] = {{row, col}, {row + 1, col}, {row + 1, col + 1}, {row, col + 1}};
          for (int diag = 0; diag < 2; ++diag)
            if (fd.n(comp.config(w, q[diag])) != fd.n(comp.config(w, q[diag + 2])))
              Put(energy, bonds, w, rows, cols, row, col, diag,
                  TenElemT(TenElemT(-t2) * ComplexConjugate(TenElemT(val[(w * np + col) * 2 + diag] / psi[w * np + col]))));   // :210 (jw applied on the device)
        }
      if (row + 2 < rows) ct.ShiftBMPSWindow(DOWN);
    }
  }
  // The diagonal hops of every plaquette with the environments of ONE row pass -- the reference's flow (square_spinless_fermion.h:
  // 161-213, square_tJ_model.h:424-463 through square_nnn_energy_solver.h:203-265: BTen2 of the row pair, ReplaceNNNSiteTrace per diagonal).  The reference's
  // graded trace carries the signs in the tensor algebra; in the decorated form a hop between a = (r, c) / (r+1, c) and
  // b = (r+1, c+1) / (r, c+1) flips the variant of every site between the two ends in row-major order -- row r right of the
  // plaquette, row r+1 left of it -- so the hopped amplitude is a replacement of the four plaquette tensors against TWISTED
  // environments: the LEFT BTen2 grown with row r+1 under flipped variants, the RIGHT BTen2 with row r flipped (second BTen2 set +
  // slice override of the C ABI).  psi of the plaquette comes from the untwisted set along the same path.
  template <typename TenElemT>
  static void Local(double t2, TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds = nullptr) {
    if (!comp.fermion) throw std::logic_error("fermionic NNN hopping needs the fermionic decoration of the component");
    const size_t n = comp.config.walkers(), rows = comp.config.rows(), cols = comp.config.cols();
    if (rows < 2 || cols < 2) return;
    const FermionDecoration &fd = *comp.fermion;
    const int32_t d = (int32_t)fd.d();
    auto &ct = comp.contractor;
    comp.SetOrder(ROW_MAJOR);
    comp.InitDevice();
    const Configuration ext = fd.ExtConfig(comp.config, ROW_MAJOR);
    auto flipped_row = [&](size_t r) {
      std::vector<int32_t> v(n * cols);
      for (size_t w = 0; w < n; ++w)
        for (size_t c = 0; c < cols; ++c) { const int32_t e = ext(w, {r, c}); v[w * cols + c] = (e / d == 0) ? e + d : e - d; }
      return v;
    };
    struct Restore {
      BMPSContractorT<TenElemT> &c;
      ~Restore() { try { c.OverrideSlice(HORIZONTAL, 0, nullptr); c.SelectBTen2Set(0); } catch (...) {} }
    } restore{ct};
    ct.GenerateBMPSApproach(UP);
    for (size_t row = 0; row + 1 < rows; ++row) {
      const std::vector<int32_t> flip0 = flipped_row(row), flip1 = flipped_row(row + 1);
      ct.SelectBTen2Set(0);
      ct.GrowFullBTen2(RIGHT, row, 2, true);
      ct.InitBTen2(LEFT, row);
      ct.SelectBTen2Set(1);
      ct.OverrideSlice(HORIZONTAL, row, &flip0);
      ct.GrowFullBTen2(RIGHT, row, 2, true);
      ct.OverrideSlice(HORIZONTAL, row + 1, &flip1);
      ct.InitBTen2(LEFT, row);
      for (size_t col = 0; col + 1 < cols; ++col) {
        const SiteIdx q[4] = {{row, col}, {row + 1, col}, {row + 1, col + 1}, {row, col + 1}};
        std::vector<int32_t> own(n * 4), cand(n * 2 * 4);
        std::vector<double> jw(n * 2, 0.0);
        bool any = false;
        for (size_t w = 0; w < n; ++w) {
          for (int k = 0; k < 4; ++k) own[w * 4 + k] = ext(w, q[k]);
          for (int diag = 0; diag < 2; ++diag) {
            const SiteIdx a = diag == 0 ? q[0] : q[1], b = diag == 0 ? q[2] : q[3];
            const bool allowed = fd.n(comp.config(w, a)) != fd.n(comp.config(w, b));      // exactly one end occupied
            if (allowed) {
              any = true;
              const size_t ia = std::min(a.r * cols + a.c, b.r * cols + b.c), ib = std::max(a.r * cols + a.c, b.r * cols + b.c);
              int between = 0;
              for (size_t x = ia + 1; x < ib; ++x) between += fd.n(comp.config(w, {x / cols, x % cols}));
              jw[w * 2 + diag] = (between & 1) ? -1.0 : 1.0;
            }
            // parity of the fermion count up to and including each plaquette site under the hopped configuration
            auto same = [](const SiteIdx &x, const SiteIdx &y) { return x.r == y.r && x.c == y.c; };
            auto st = [&](const SiteIdx &s) { return same(s, a) ? comp.config(w, b) : (same(s, b) ? comp.config(w, a) : comp.config(w, s)); };
            // count before (row, col): inclusive parity of ext at (row, col) minus its own occupation
            const int p00 = (ext(w, q[0]) / d) ^ fd.n(comp.config(w, q[0]));          // fermions strictly before (row, col)
            // row `row`: between (row, col+1) and the end, and row+1 up to col-1: unchanged occupations
            int mid = 0;                                                               // fermions strictly between (row, col+1) and (row+1, col)
            for (size_t c2 = col + 2; c2 < cols; ++c2) mid ^= fd.n(comp.config(w, {row, c2}));
            for (size_t c2 = 0; c2 < col; ++c2) mid ^= fd.n(comp.config(w, {row + 1, c2}));
            const int n0 = fd.n(st(q[0])), n3 = fd.n(st(q[3])), n1 = fd.n(st(q[1])), n2 = fd.n(st(q[2]));
            const int i0 = p00 ^ n0, i3 = i0 ^ n3, i1 = i3 ^ mid ^ n1, i2 = i1 ^ n2;
            int32_t *cd = &cand[(w * 2 + diag) * 4];
            cd[0] = st(q[0]) + d * i0; cd[1] = st(q[1]) + d * i1; cd[2] = st(q[2]) + d * i2; cd[3] = st(q[3]) + d * i3;
          }
        }
        if (any) {
          const std::vector<TenElemT> psi = ct.ReplacePlaquetteTrace(q[0], 1, own, 0, 0);
          const std::vector<TenElemT> psi_ex = ct.ReplacePlaquetteTrace(q[0], 2, cand, 1, 1);
          for (size_t w = 0; w < n; ++w)
            for (int diag = 0; diag < 2; ++diag)
              if (jw[w * 2 + diag] != 0.0)
                Put(energy, bonds, w, rows, cols, row, col, diag,
                    TenElemT(TenElemT(-t2 * jw[w * 2 + diag]) * ComplexConjugate(TenElemT(psi_ex[w * 2 + diag] / psi[w]))));   // :210
        }
        if (col + 2 < cols) {      // both LEFT chains advance over column col (set 1 under the row+1 override)
          ct.GrowBTen2Step(LEFT, row);
          ct.SelectBTen2Set(0);
          ct.OverrideSlice(HORIZONTAL, row + 1, nullptr);
          ct.GrowBTen2Step(LEFT, row);
          ct.SelectBTen2Set(1);
          ct.OverrideSlice(HORIZONTAL, row + 1, &flip1);
        }
      }
      ct.OverrideSlice(HORIZONTAL, row + 1, nullptr);
      ct.SelectBTen2Set(0);
      if (row + 2 < rows) ct.ShiftBMPSWindow(DOWN);
    }
  }
  // sum over the plaquette diagonals of -t2 * jw * psi(S with the two sites exchanged) / psi(S); jw = (-1)^(fermions strictly
  // between the two sites in row-major order).  Leaves comp on its original configuration.
  template <typename TenElemT>
  static void Fresh(double t2, TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds = nullptr) {
    if (!comp.fermion) throw std::logic_error("fermionic NNN hopping needs the fermionic decoration of the component");
    const size_t n = comp.config.walkers(), rows = comp.config.rows(), cols = comp.config.cols();
    const Configuration orig = comp.config;
    comp.ReplaceGlobalConfig(orig);                       // psi of the original configuration, fresh (row-major order)
    const std::vector<TenElemT> psi0 = comp.amplitude;
    for (size_t row = 0; row + 1 < rows; ++row)
      for (size_t col = 0; col + 1 < cols; ++col)
        for (int diag = 0; diag < 2; ++diag) {
          const SiteIdx a = diag == 0 ? SiteIdx{row, col} : SiteIdx{row + 1, col};
          const SiteIdx b = diag == 0 ? SiteIdx{row + 1, col + 1} : SiteIdx{row, col + 1};
          bool any = false;
          for (size_t w = 0; w < n; ++w) any |= comp.fermion->n(orig(w, a)) != comp.fermion->n(orig(w, b));
          if (!any) continue;
          Configuration hop = orig;
          for (size_t w = 0; w < n; ++w) { hop(w, a) = orig(w, b); hop(w, b) = orig(w, a); }
          comp.ReplaceGlobalConfig(hop);
          const size_t ia = std::min(a.r * cols + a.c, b.r * cols + b.c), ib = std::max(a.r * cols + a.c, b.r * cols + b.c);
          for (size_t w = 0; w < n; ++w) {
            if (comp.fermion->n(orig(w, a)) == comp.fermion->n(orig(w, b))) continue;
            int between = 0;
            for (size_t q = ia + 1; q < ib; ++q) between += comp.fermion->n(orig(w, {q / cols, q % cols}));
            Put(energy, bonds, w, rows, cols, row, col, diag,
                TenElemT(TenElemT(-t2 * ((between & 1) ? -1.0 : 1.0)) * ComplexConjugate(TenElemT(comp.amplitude[w] / psi0[w]))));
          }
        }
    comp.ReplaceGlobalConfig(orig);
  }
};

// square_spinless_fermion.h:51-200: H = -t sum_<ij> (c+_i c_j + h.c.) - t2 sum_<<ij>> (c+_i c_j + h.c.) + V sum_<ij> n_i n_j.
// psi is recomputed with Trace next to psi' (same contraction path, docs/dev/design/math/
// fermion-sign-in-bmps-contraction.md), the bosonic inv_psi argument is unused.  NNN hopping (:161-200): FermionNNNHop above.
class SquareSpinlessFermion : public SquareNNModelEnergySolver<SquareSpinlessFermion>,
                              public SquareNNNModelMeasurementSolver<SquareSpinlessFermion> {
 public:
  static constexpr bool kFermionicModel = true;
  static constexpr bool requires_density_measurement = true;   // :55-56
  static constexpr bool requires_spin_sz_measurement = false;
  // the diagonal hops of the measurement registry: added to `energy`, per diagonal into `bonds` (FermionNNNHop)
  template <typename TenElemT>
  void FermionNNNBondEnergies(TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds) const {
    FermionNNNHop::Add(t2_, comp, energy, bonds);
  }
  SquareSpinlessFermion(double t, double V) : t_(t), t2_(0.0), V_(V) {}
  SquareSpinlessFermion(double t, double t2, double V) : t_(t), t2_(t2), V_(V) {}
  template <bool calchols = true, typename TenElemT = double>
  EnergyAndHolesT<TenElemT> CalEnergyAndHoles(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp,
                                              bool holes_on_device = false) {
    EnergyAndHolesT<TenElemT> out =
        SquareNNModelEnergySolver<SquareSpinlessFermion>::template CalEnergyAndHoles<calchols, TenElemT>(sitps, comp, holes_on_device);
    FermionNNNHop::Add(t2_, comp, out.energy);
    return out;
  }
  double CalDensityImpl(int32_t config) const { return double(1 - config); }   // :95-97
  template <typename TenElemT>
  std::vector<TenElemT> EvaluateBondEnergy(const SiteIdx &s1, const SiteIdx &s2, BondOrientation orient,
                                           TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &) {   // :134-159
    const size_t n = comp.config.walkers();
    std::vector<int32_t> cand(n * 2);
    std::vector<TenElemT> e(n);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      cand[2 * w] = comp.config(w, s2);
      cand[2 * w + 1] = comp.config(w, s1);
      any |= cand[2 * w] != cand[2 * w + 1];
      e[w] = V_ * CalDensityImpl(comp.config(w, s1)) * CalDensityImpl(comp.config(w, s2));
    }
    if (!any) return e;
    std::vector<TenElemT> psi = comp.contractor.Trace(s1, orient);
    std::vector<TenElemT> psi_ex = comp.ReplaceNNSiteTrace(s1, s2, orient, 1, cand);
    for (size_t w = 0; w < n; ++w)
      if (comp.config(w, s1) != comp.config(w, s2)) e[w] += -t_ * ComplexConjugate(TenElemT(psi_ex[w] / psi[w]));   // :156
    return e;
  }
  // EvaluateBondEnergy of one walker from ratio = ComplexConjugate(psi_ex / psi) (the device-side energy slice)
  static constexpr bool kExchangeBondEnergy = true;
  static constexpr bool kExchangeBondPsiPerBond = true;
  template <typename TenElemT>
  TenElemT BondEnergyFromExchange(int32_t config1, int32_t config2, TenElemT ratio) const {
    TenElemT e = V_ * CalDensityImpl(config1) * CalDensityImpl(config2);
    if (config1 != config2) e += -t_ * ratio;
    return e;
  }
  double EvaluateTotalOnsiteEnergy(const Configuration &, size_t) const { return 0.0; }   // :92
 private:
  double t_, t2_, V_;
};

// SingletPairCorrelationMixin (base/singlet_pair_correlation_measurement_mixin.h): SC_singlet_pair_corr, the pair-pair correlation
// <Delta+(ref bond) Delta(target bond)> between the horizontal reference bond (y1, x1)-(y1, x1 + 1) and every horizontal target bond
// (y2, x2)-(y2, x2 + 1) with y2 > y1; t-J states 0 up, 1 down, 2 empty.  The reference's MeasureSingletPairCorrelation throws ("Fermion
// sign is NOT correctly handled", :279-297: its graded contraction traces out the parity indices); the algorithm below the throw
// (:349-534) runs here unchanged, because a fermionic state is an ordinary contraction of sign-decorated components times
// Sigma(N_f) and both bonds are pairs of modes adjacent in the row-major order: a pair move changes the components of its two sites
// only and keeps the parity behind them, so the rows below need no change.
//   value = 1/2 conj(rho_ud - rho_du) * (+1 for a target (up, down), -1 for (down, up)),
//   rho_x = psi(S with ref -> x, target -> (empty, empty)) / psi(S) = (-1)(-1) excited trace / original trace
// for an (empty, empty) reference bond and an (up, down) / (down, up) target, 0 otherwise: Sigma(S') / Sigma(S) is -1 for the
// injection and -1 for the removal.  tests/test_cpu_pair_corr.py pins the value to the dense Delta+_ref Delta_tgt.
// Schedule: per reference bond two excited walkers forked from up_stack[y1] and evolved through the row with the pair injected; the
// original walker (psi(S) along the same path, so that truncation errors cancel in the ratio) is shared by the reference bonds of
// one y1 -- its numbers do not depend on x1.  A reference bond that is (empty, empty) for no walker of the batch creates no walker.
// Device slices: SetMPOExcitedPair + ONE PairTraceSlice per walker and target row; PEPSHOST_NO_DEVICE_SWEEP=1: SetMPOStates,
// InitBTenLeft / InitBTenRight, TraceWithTwoSiteBTen, ShiftBTenWindow.
template <class Model>
class SingletPairCorrelationMixin {
 public:
  void SetEnableSingletPairCorrelation(bool enable) { enable_singlet_pair_correlation_ = enable; }
  bool IsSingletPairCorrelationEnabled() const { return enable_singlet_pair_correlation_; }
  void SetSelectedRefBonds(std::vector<std::pair<size_t, size_t>> bonds) { selected_ref_bonds_ = std::move(bonds); }   // (y, x) of the left site
  const std::vector<std::pair<size_t, size_t>> &GetSelectedRefBonds() const { return selected_ref_bonds_; }
  // the reference bonds measured, in output order (:193-212): all of them, or the selection without its out-of-lattice members sorted
  static std::vector<std::pair<size_t, size_t>> ValidRefBonds(size_t Ly, size_t Lx, const std::vector<std::pair<size_t, size_t>> &ref_bonds = {}) {
    std::vector<std::pair<size_t, size_t>> out;
    if (Ly < 2 || Lx < 2) return out;
    if (ref_bonds.empty()) {
      for (size_t y1 = 0; y1 + 1 < Ly; ++y1)
        for (size_t x1 = 0; x1 + 1 < Lx; ++x1) out.emplace_back(y1, x1);
      return out;
    }
    for (const auto &b : ref_bonds)
      if (b.first < Ly - 1 && b.second < Lx - 1) out.push_back(b);
    std::sort(out.begin(), out.end());
    return out;
  }
  static size_t ComputeNumSCPairs(size_t Ly, size_t Lx, const std::vector<std::pair<size_t, size_t>> &ref_bonds = {}) {   // :136-160
    size_t count = 0;
    for (const auto &b : ValidRefBonds(Ly, Lx, ref_bonds)) count += (Ly - 1 - b.first) * (Lx - 1);
    return count;
  }
  // {ref_y, ref_x, 0, tgt_y, tgt_x, 0} per value (:176-215)
  static std::vector<std::array<size_t, 6>> GenerateSCPairCorrIndexMapping(size_t Ly, size_t Lx,
                                                                           const std::vector<std::pair<size_t, size_t>> &ref_bonds = {}) {
    std::vector<std::array<size_t, 6>> mapping;
    for (const auto &b : ValidRefBonds(Ly, Lx, ref_bonds))
      for (size_t y2 = b.first + 1; y2 < Ly; ++y2)
        for (size_t x2 = 0; x2 + 1 < Lx; ++x2) mapping.push_back({b.first, b.second, 0, y2, x2, 0});
    return mapping;
  }
  static std::string GenerateSCPairCorrCoordString(size_t Ly, size_t Lx, const std::vector<std::pair<size_t, size_t>> &ref_bonds = {}) {   // :233-245
    const auto mapping = GenerateSCPairCorrIndexMapping(Ly, Lx, ref_bonds);
    std::ostringstream oss;
    oss << "# idx ref_y ref_x ref_orient tgt_y tgt_x tgt_orient\n";
    for (size_t i = 0; i < mapping.size(); ++i) {
      const auto &m = mapping[i];
      oss << i << " " << m[0] << " " << m[1] << " " << m[2] << " " << m[3] << " " << m[4] << " " << m[5] << "\n";
    }
    return oss.str();
  }
  void DescribeSingletPairCorrelation(std::vector<ObservableMeta> &out, size_t ly, size_t lx) const {   // square_tJ_model.h:677-683
    if (!enable_singlet_pair_correlation_) return;
    const auto ref_bonds = selected_ref_bonds_;
    out.push_back({"SC_singlet_pair_corr", "Singlet pair correlation <Delta^dag Delta> values.", {ComputeNumSCPairs(ly, lx, ref_bonds)},
                   {"pair_idx"}, [ref_bonds](size_t ly_, size_t lx_) { return GenerateSCPairCorrCoordString(ly_, lx_, ref_bonds); }});
  }
  // pair tables over physical states ([3 * 3][2][2], (-1, -1) for none): Delta+ on an (empty, empty) bond (slot 0 (up, down), slot 1
  // (down, up)); Delta on an (up, down) / (down, up) bond (slot 0); the identity on those two (slot 0: psi_original)
  static std::vector<int32_t> PairTableOf(int kind) {
    std::vector<int32_t> tab(9 * 4, -1);
    auto set = [&](int a, int b, int k, int pa, int pb) { tab[((a * 3 + b) * 2 + k) * 2] = pa; tab[((a * 3 + b) * 2 + k) * 2 + 1] = pb; };
    if (kind == 0) { set(2, 2, 0, 0, 1); set(2, 2, 1, 1, 0); }
    else if (kind == 1) { set(0, 1, 0, 2, 2); set(1, 0, 0, 2, 2); }
    else { set(0, 1, 0, 0, 1); set(1, 0, 0, 1, 0); }
    return tab;
  }
  // The component is in ROW_MAJOR order, the UP stack reaches the last reference row and the DOWN stack is full.
  template <typename TenElemT>
  void MeasureSingletPairCorrelation(TPSWaveFunctionComponentT<TenElemT> &comp, ObservableMapT<TenElemT> &out) const {
    if (!enable_singlet_pair_correlation_) return;
    auto &c = comp.contractor;
    const size_t Ly = c.rows(), Lx = c.cols(), n = comp.config.walkers();
    const auto bonds = ValidRefBonds(Ly, Lx, selected_ref_bonds_);
    if (bonds.empty()) { out.make("SC_singlet_pair_corr", 0); return; }   // (the key DescribeObservables announces, with its shape {0})
    if (!comp.fermion || comp.order != ROW_MAJOR)
      throw std::logic_error("MeasureSingletPairCorrelation: needs the fermionic decoration in row-major order");
    const FermionDecoration &fd = *comp.fermion;
    if (fd.d() != 3) throw std::logic_error("MeasureSingletPairCorrelation: the t-J states (up, down, empty) are expected");
    const size_t per = ComputeNumSCPairs(Ly, Lx, selected_ref_bonds_), np = Lx - 1, d = fd.d();
    auto &corr = out.make("SC_singlet_pair_corr", per);
    const size_t max_ref_y = bonds.back().first, n_up = c.BMPSStackSize(UP), n_down = c.BMPSStackSize(DOWN);
    if (n_up <= max_ref_y)
      throw std::runtime_error("MeasureSingletPairCorrelation: UP BMPS stack insufficient. Need depth " + std::to_string(max_ref_y + 1) +
                               ", got " + std::to_string(n_up) +
                               ". Call contractor.GrowFullBMPS(tn, UP) after setting truncation params before measurement.");
    const bool dev_slice = DeviceSlicesEnabled();
    std::vector<int32_t> occ(fd.d());
    for (size_t s = 0; s < occ.size(); ++s) occ[s] = fd.n((int32_t)s);
    const std::vector<int32_t> inject = PairTableOf(0), remove = PairTableOf(1), ident = PairTableOf(2);
    auto is_pair = [&](size_t w, size_t y, size_t x) {
      const int32_t a = comp.config(w, {y, x}), b = comp.config(w, {y, x + 1});
      return (a == 0 && b == 1) || (a == 1 && b == 0);
    };
    // slot 0 of the scan of row y2 for the walkers of `mask`: sign * two-site trace [w][x2], 0 where the table has no candidate
    auto scan_row = [&](typename BMPSContractorT<TenElemT>::BMPSWalker &walker, size_t y2, const std::vector<int32_t> &table,
                        const std::vector<uint8_t> &mask) {
      const size_t bottom = Ly - 1 - y2;
      if (bottom >= n_down)
        throw std::runtime_error("MeasureSingletPairCorrelation: DOWN BMPS stack insufficient. Need depth " + std::to_string(bottom + 1) +
                                 ", got " + std::to_string(n_down) +
                                 ". Call contractor.GrowFullBMPS(tn, DOWN) after setting truncation params before measurement.");
      walker.SetMPO(y2);
      std::vector<TenElemT> row(n * np, TenElemT(0.0));
      if (dev_slice) {
        const std::vector<TenElemT> both = walker.PairTraceSlice(bottom, occ, table, mask);
        for (size_t k = 0; k < n * np; ++k) row[k] = both[2 * k];
      } else {
        const DeviceTraceScaling<TenElemT> scaling(c);          // (scaled as the slice scales them: the same bytes on both paths)
        walker.InitBTenLeft(bottom, 0);
        walker.InitBTenRight(bottom, 1);
        for (size_t x2 = 0; x2 < np; ++x2) {
          const SiteIdx s1{y2, x2}, s2{y2, x2 + 1};
          std::vector<int32_t> cand(n * 2);
          std::vector<int> sign(n, 0);
          bool any = false;
          for (size_t w = 0; w < n; ++w) {
            const int32_t a = comp.config(w, s1), b = comp.config(w, s2);
            const int32_t pa = table[((a * d + b) * 2) * 2], pb = table[((a * d + b) * 2) * 2 + 1];
            cand[2 * w] = pa < 0 ? a : pa;
            cand[2 * w + 1] = pa < 0 ? b : pb;
            if (pa >= 0 && mask[w]) { sign[w] = fd.n(pa) + fd.n(pb) == fd.n(a) + fd.n(b) ? 1 : -1; any = true; }
          }
          if (any) {
            const std::vector<TenElemT> tr = walker.TraceWithTwoSiteBTen(bottom, x2, comp.DeviceStatesNN(s1, s2, 1, cand));
            for (size_t w = 0; w < n; ++w)
              if (sign[w]) row[w * np + x2] = TenElemT(double(sign[w]) * tr[w]);
          }
          if (x2 + 1 < np) walker.ShiftBTenWindow(bottom, RIGHT);
        }
      }
      walker.ClearBTen();
      return row;
    };
    // all target rows of a walker that has absorbed the rows [0, y1]
    auto scan_rows = [&](typename BMPSContractorT<TenElemT>::BMPSWalker &walker, size_t y1, const std::vector<int32_t> &table,
                         const std::vector<uint8_t> &mask) {
      std::vector<std::vector<TenElemT>> rows;
      for (size_t y2 = y1 + 1; y2 < Ly; ++y2) {
        if (y2 > y1 + 1) { walker.SetMPO(y2 - 1); walker.Evolve(); }
        rows.push_back(scan_row(walker, y2, table, mask));
      }
      return rows;
    };
    const std::vector<uint8_t> everyone(n, 1);
    std::vector<std::vector<TenElemT>> psi_orig;
    size_t psi_y1 = Ly, pos = 0;
    for (const auto &bond : bonds) {
      const size_t y1 = bond.first, x1 = bond.second, npair = (Ly - 1 - y1) * np;
      std::vector<uint8_t> ref_valid(n);
      bool any = false;
      for (size_t w = 0; w < n; ++w) {
        ref_valid[w] = comp.config(w, {y1, x1}) == 2 && comp.config(w, {y1, x1 + 1}) == 2;
        any |= ref_valid[w] != 0;
      }
      if (!any) { pos += npair; continue; }
      if (psi_y1 != y1) {
        auto original_walker = c.MakeWalker(UP, y1);
        original_walker.SetMPO(y1);
        original_walker.Evolve();
        psi_orig = scan_rows(original_walker, y1, ident, everyone);
        psi_y1 = y1;
      }
      std::vector<std::vector<TenElemT>> over[2];
      for (int k = 0; k < 2; ++k) {
        auto excited_walker = c.MakeWalker(UP, y1);
        if (dev_slice) {
          excited_walker.SetMPOExcitedPair(y1, x1, occ, inject, k);
        } else {
          Configuration changed = comp.config;
          for (size_t w = 0; w < n; ++w)
            if (ref_valid[w]) { changed(w, {y1, x1}) = k == 0 ? 0 : 1; changed(w, {y1, x1 + 1}) = k == 0 ? 1 : 0; }
          const Configuration ext = fd.ExtConfig(changed, ROW_MAJOR);
          std::vector<int32_t> excited(n * Lx);
          for (size_t w = 0; w < n; ++w)
            for (size_t x = 0; x < Lx; ++x) excited[w * Lx + x] = ext(w, {y1, x});
          excited_walker.SetMPOStates(y1, excited);
        }
        excited_walker.Evolve();
        over[k] = scan_rows(excited_walker, y1, remove, ref_valid);
      }
      for (size_t y2 = y1 + 1; y2 < Ly; ++y2) {
        const size_t r = y2 - y1 - 1;
        for (size_t w = 0; w < n; ++w)
          for (size_t x2 = 0; x2 < np; ++x2) {
            if (!ref_valid[w] || !is_pair(w, y2, x2)) continue;
            const TenElemT psi = psi_orig[r][w * np + x2];
            if (psi == TenElemT(0.0))
              throw std::runtime_error("MeasureSingletPairCorrelation: psi_original = 0 for sampled configuration. "
                                       "This indicates a bug in sampling or tensor network contraction.");
            // (the removal's sign is in the scan; the injection's -1 here)
            const TenElemT ratio_ud = TenElemT(-over[0][r][w * np + x2] / psi), ratio_du = TenElemT(-over[1][r][w * np + x2] / psi);
            const double tgt = comp.config(w, {y2, x2}) == 0 ? 1.0 : -1.0;
            corr[w * per + pos + r * np + x2] = TenElemT(0.5 * tgt) * ComplexConjugate(TenElemT(ratio_ud - ratio_du));
          }
      }
      pos += npair;
    }
  }

 protected:
  bool enable_singlet_pair_correlation_ = false;
  std::vector<std::pair<size_t, size_t>> selected_ref_bonds_;
};

// square_tJ_model.h:301-345 (SquaretJModelMixIn::EvaluateBondEnergy) + :215-228: states 0 up, 1 down, 2 empty
// (vmc_basic/tj_single_site_state.h:19-23); H = -t sum (c+ c + h.c.) + J sum (S.S - n n / 4) + V sum n n - mu N.
// NNN hopping t2 (:424-463): FermionNNNHop above.
// Measurement (:546-603, :657-850): the registry of the diagonal-bond traversal with spin_z, charge and the bond-singlet pairing order
//   Delta+_ij = (c+_i,up c+_j,down - c+_i,down c+_j,up) / sqrt(2)   on the NN bond with i the left / upper, j the right / lower site,
// in the basis |S> = product of c+ over the occupied sites in row-major order.  SC_singlet_pair_corr: the mixin above, off by default
// (SquaretJNNModel and SquaretJNNNModel inherit it).
class SquaretJVModel : public SquareNNModelEnergySolver<SquaretJVModel>, public SquareNNNModelMeasurementSolver<SquaretJVModel>,
                       public SingletPairCorrelationMixin<SquaretJVModel> {
 public:
  static constexpr bool kFermionicModel = true;
  static constexpr bool requires_spin_sz_measurement = true;
  static constexpr bool requires_density_measurement = true;
  static constexpr bool enable_sc_measurement = true;
  double CalSpinSzImpl(int32_t config) const { return config == 0 ? 0.5 : (config == 1 ? -0.5 : 0.0); }
  double CalDensityImpl(int32_t config) const { return config == 2 ? 0.0 : 1.0; }
  template <typename TenElemT>
  void FermionNNNBondEnergies(TPSWaveFunctionComponentT<TenElemT> &comp, std::vector<TenElemT> &energy, std::vector<TenElemT> *bonds) const {
    FermionNNNHop::Add(t2_, comp, energy, bonds);
  }
  // The configurations a pair operator connects the states (a, b) of a bond to, [3 * 3][2][2] over physical states ((-1, -1): none):
  // (empty, empty) -> (up, down), (down, up);  (up, down) and (down, up) -> (empty, empty).  The pair table of
  // pepsgpu_nn_pair_slice_fermion.
  static std::vector<int32_t> PairTable() {
    std::vector<int32_t> tab(9 * 4, -1);
    auto set = [&](int a, int b, int k, int pa, int pb) { tab[((a * 3 + b) * 2 + k) * 2] = pa; tab[((a * 3 + b) * 2 + k) * 2 + 1] = pb; };
    set(2, 2, 0, 0, 1);
    set(2, 2, 1, 1, 0);
    set(0, 1, 0, 2, 2);
    set(1, 0, 0, 2, 2);
    return tab;
  }
  // (delta_dag, delta) of one bond (:569-602) from rho_k = jw psi(S'_k) / psi(S) of its two candidates of PairTable
  template <typename TenElemT>
  static std::pair<TenElemT, TenElemT> BondSCFromPairs(int32_t c1, int32_t c2, TenElemT rho0, TenElemT rho1) {
    const double isq2 = 1.0 / std::sqrt(2.0);
    if (c1 == 2 && c2 == 2) return {TenElemT(ComplexConjugate(TenElemT(rho0 - rho1)) * isq2), TenElemT(0.0)};
    if (c1 == 0 && c2 == 1) return {TenElemT(0.0), TenElemT(ComplexConjugate(rho0) * isq2)};
    if (c1 == 1 && c2 == 0) return {TenElemT(0.0), TenElemT(-ComplexConjugate(rho0) * isq2)};
    return {TenElemT(0.0), TenElemT(0.0)};
  }
  // EvaluateBondSC (:195-212): Trace + ONE ReplaceNNSiteTrace over the two candidates of the bond.  The ratio of the decorated
  // contractions misses Sigma(S') / Sigma(S), which is -1 for a candidate that changes the electron number by +-2.
  template <typename TenElemT>
  std::vector<std::pair<TenElemT, TenElemT>> EvaluateBondSC(const SiteIdx &s1, const SiteIdx &s2, BondOrientation orient,
                                                            TPSWaveFunctionComponentT<TenElemT> &comp) const {
    const size_t n = comp.config.walkers();
    const FermionDecoration &fd = *comp.fermion;
    const std::vector<int32_t> tab = PairTable();
    std::vector<int32_t> cand(n * 4);
    std::vector<int> sign(n * 2, 0);
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      const int32_t c1 = comp.config(w, s1), c2 = comp.config(w, s2);
      for (int k = 0; k < 2; ++k) {
        const int32_t pa = tab[((c1 * 3 + c2) * 2 + k) * 2], pb = tab[((c1 * 3 + c2) * 2 + k) * 2 + 1];
        cand[(w * 2 + k) * 2] = pa < 0 ? c1 : pa;
        cand[(w * 2 + k) * 2 + 1] = pa < 0 ? c2 : pb;
        if (pa >= 0) { sign[w * 2 + k] = fd.n(pa) + fd.n(pb) == fd.n(c1) + fd.n(c2) ? 1 : -1; any = true; }
      }
    }
    std::vector<std::pair<TenElemT, TenElemT>> out(n, {TenElemT(0.0), TenElemT(0.0)});
    if (!any) return out;
    const std::vector<TenElemT> psi = comp.contractor.Trace(s1, orient);
    const std::vector<TenElemT> psi_ex = comp.ReplaceNNSiteTrace(s1, s2, orient, 2, cand);
    for (size_t w = 0; w < n; ++w) {
      if (sign[w * 2] == 0 && sign[w * 2 + 1] == 0) continue;
      if (psi[w] == TenElemT(0.0)) throw std::runtime_error("EvaluateBondSingletPairFortJModel: psi is zero.");
      TenElemT rho[2];
      for (int k = 0; k < 2; ++k) rho[k] = sign[w * 2 + k] ? TenElemT(double(sign[w * 2 + k]) * psi_ex[w * 2 + k] / psi[w]) : TenElemT(0.0);
      out[w] = BondSCFromPairs(comp.config(w, s1), comp.config(w, s2), rho[0], rho[1]);
    }
    return out;
  }
  SquaretJVModel(double t, double t2, double J, double V, double mu) : t_(t), t2_(t2), J_(J), V_(V), mu_(mu) {}
  template <bool calchols = true, typename TenElemT = double>
  EnergyAndHolesT<TenElemT> CalEnergyAndHoles(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp,
                                              bool holes_on_device = false) {
    EnergyAndHolesT<TenElemT> out =
        SquareNNModelEnergySolver<SquaretJVModel>::template CalEnergyAndHoles<calchols, TenElemT>(sitps, comp, holes_on_device);
    FermionNNNHop::Add(t2_, comp, out.energy);
    return out;
  }
  template <typename TenElemT>
  std::vector<TenElemT> EvaluateBondEnergy(const SiteIdx &s1, const SiteIdx &s2, BondOrientation orient,
                                           TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &) {
    const size_t n = comp.config.walkers();
    std::vector<int32_t> cand(n * 2);
    std::vector<TenElemT> e(n, TenElemT(0.0));
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      const int32_t c1 = comp.config(w, s1), c2 = comp.config(w, s2);
      cand[2 * w] = c2;
      cand[2 * w + 1] = c1;
      if (c1 == c2) e[w] = (c1 == 2) ? 0.0 : V_;            // both empty / parallel spins: sz sz - n n / 4 = 0   (:312-318)
      else any = true;
    }
    if (!any) return e;
    std::vector<TenElemT> psi = comp.contractor.Trace(s1, orient);
    std::vector<TenElemT> psi_ex = comp.ReplaceNNSiteTrace(s1, s2, orient, 1, cand);
    for (size_t w = 0; w < n; ++w) {
      const int32_t c1 = comp.config(w, s1), c2 = comp.config(w, s2);
      if (c1 == c2) continue;
      const TenElemT ratio = ComplexConjugate(TenElemT(psi_ex[w] / psi[w]));
      e[w] = (c1 == 2 || c2 == 2) ? TenElemT(-t_ * ratio) : TenElemT((-0.5 + 0.5 * ratio) * J_ + V_);      // :334-343
    }
    return e;
  }
  // EvaluateBondEnergy of one walker from ratio = ComplexConjugate(psi_ex / psi) (the device-side energy slice)
  static constexpr bool kExchangeBondEnergy = true;
  static constexpr bool kExchangeBondPsiPerBond = true;
  template <typename TenElemT>
  TenElemT BondEnergyFromExchange(int32_t c1, int32_t c2, TenElemT ratio) const {
    if (c1 == c2) return TenElemT((c1 == 2) ? 0.0 : V_);
    return (c1 == 2 || c2 == 2) ? TenElemT(-t_ * ratio) : TenElemT((-0.5 + 0.5 * ratio) * J_ + V_);
  }
  double EvaluateTotalOnsiteEnergy(const Configuration &config, size_t w) const {   // :215-228
    if (mu_ == 0.0) return 0.0;
    size_t ele = 0;
    for (size_t r = 0; r < config.rows(); ++r)
      for (size_t c = 0; c < config.cols(); ++c) ele += config(w, {r, c}) != 2;
    return -mu_ * double(ele);
  }
 private:
  double t_, t2_, J_, V_, mu_;
};
// square_tJ_model.h:613-705: the named models hand V = 0 (and SquaretJNNModel t2 = 0) to the mix-in
// (SquaretJNNModel measures with the nearest-neighbour form, :613-705: no diagonal-bond keys)
class SquaretJNNModel : public SquaretJVModel, public SquareNNModelMeasurementSolver<SquaretJNNModel> {
 public:
  using SquareNNModelMeasurementSolver<SquaretJNNModel>::EvaluateObservables;
  using SquareNNModelMeasurementSolver<SquaretJNNModel>::EvaluatePsiSummary;
  using SquareNNModelMeasurementSolver<SquaretJNNModel>::EvaluatePsiSummaryT;
  using SquareNNModelMeasurementSolver<SquaretJNNModel>::DescribeObservables;
  SquaretJNNModel(double t, double J, double mu) : SquaretJVModel(t, 0.0, J, 0.0, mu) {}
};
class SquaretJNNNModel : public SquaretJVModel {
 public:
  SquaretJNNNModel(double t, double t2, double J, double mu) : SquaretJVModel(t, t2, J, 0.0, mu) {}
};

// square_hubbard_model.h:76-263: H = -t sum_<ij>,s (c+_is c_js + h.c.) + U sum_i n_iup n_idown - mu sum_is n_is; states 0 up-down, 1 up,
// 2 down, 3 empty (:18-23), fermion parities [0, 1, 1, 0].  EvaluateBondEnergy (:190-262) in one rule: site 1 is the earlier site of the
// bond in the mode order of the pass (left / upper), a bond contributes -t sum_sigma s_sigma ComplexConjugate(psi'_sigma / psi) with
// psi'_sigma the amplitude with the sigma electron hopped across the bond (at most one per sigma) and s_up = (-1)^(n_down of site 1),
// s_down = (-1)^(n_up of site 2): the occupation of the one mode the hop passes in the order (1 up, 1 down, 2 up, 2 down).  The six
// branches of the reference are this table; tests/test_cpu_hubbard.py pins it to a dense Jordan-Wigner Hamiltonian.
class SquareHubbardModel : public SquareNNModelEnergySolver<SquareHubbardModel>, public SquareNNModelMeasurementSolver<SquareHubbardModel> {
 public:
  static constexpr bool kFermionicModel = true;
  static constexpr bool requires_density_measurement = true;   // :80-81
  static constexpr bool requires_spin_sz_measurement = true;
  static constexpr bool kHopBondEnergy = true;
  SquareHubbardModel(double t, double U, double mu) : t_(t), U_(U), mu_(mu) {}
  double CalDensityImpl(int32_t config) const { return HubbardConfig2Density((size_t)config); }   // :119-121
  double CalSpinSzImpl(int32_t config) const { return HubbardConfig2Spinz((size_t)config); }      // :123-125
  // slot 0: the up electron hopped, slot 1: the down electron hopped; [16][2][2] over physical states, (-1, -1) for none
  static std::vector<int32_t> HopTable() {
    std::vector<int32_t> tab(16 * 4, -1);
    static const int32_t state_of[2][2] = {{3, 2}, {1, 0}};          // [n_up][n_down]
    for (size_t a = 0; a < 4; ++a)
      for (size_t b = 0; b < 4; ++b) {
        const auto na = HubbardConfig2SpinCounts(a), nb = HubbardConfig2SpinCounts(b);
        int32_t *row = tab.data() + (a * 4 + b) * 4;
        if (na.first != nb.first) { row[0] = state_of[nb.first][na.second]; row[1] = state_of[na.first][nb.second]; }
        if (na.second != nb.second) { row[2] = state_of[na.first][nb.second]; row[3] = state_of[nb.first][na.second]; }
      }
    return tab;
  }
  // the bond energy of one walker from r_k = ComplexConjugate(psi'_k / psi) of the two slots of HopTable (a slot without a hop adds nothing)
  template <typename TenElemT>
  TenElemT BondEnergyFromHops(int32_t c1, int32_t c2, TenElemT r_up, TenElemT r_dn) const {
    const auto n1 = HubbardConfig2SpinCounts((size_t)c1), n2 = HubbardConfig2SpinCounts((size_t)c2);
    TenElemT e(0.0);
    if (n1.first != n2.first) e += TenElemT((n1.second ? t_ : -t_) * r_up);        // -t s_up, s_up = (-1)^(n_down of site 1)
    if (n1.second != n2.second) e += TenElemT((n2.first ? t_ : -t_) * r_dn);       // -t s_down, s_down = (-1)^(n_up of site 2)
    return e;
  }
  // :190-262 batched over the walkers: Trace + ONE ReplaceNNSiteTrace over the two candidate slots (a walker without candidate k keeps
  // its own pair there); nothing for a bond on which every walker has equal states (:200-202)
  template <typename TenElemT>
  std::vector<TenElemT> EvaluateBondEnergy(const SiteIdx &s1, const SiteIdx &s2, BondOrientation orient,
                                           TPSWaveFunctionComponentT<TenElemT> &comp, const std::vector<TenElemT> &) {
    const size_t n = comp.config.walkers();
    const FermionDecoration &fd = *comp.fermion;
    const std::vector<int32_t> tab = HopTable();
    std::vector<int32_t> cand(n * 4);
    std::vector<double> sign(n * 2, 0.0);
    std::vector<TenElemT> e(n, TenElemT(0.0));
    bool any = false;
    for (size_t w = 0; w < n; ++w) {
      const int32_t c1 = comp.config(w, s1), c2 = comp.config(w, s2);
      for (int k = 0; k < 2; ++k) {
        const int32_t pa = tab[(size_t)(c1 * 4 + c2) * 4 + 2 * k], pb = tab[(size_t)(c1 * 4 + c2) * 4 + 2 * k + 1];
        cand[(w * 2 + k) * 2] = pa < 0 ? c1 : pa;
        cand[(w * 2 + k) * 2 + 1] = pa < 0 ? c2 : pb;
        // Sigma(S') / Sigma(S), which the ratio of the decorated contractions misses: -1 where the hop changes the number of odd
        // sites by +-2, (up-down, empty) <-> (up, down) -- what pepsgpu_nn_hop_slice_fermion applies on the device
        if (pa >= 0) { sign[w * 2 + k] = fd.n(pa) + fd.n(pb) == fd.n(c1) + fd.n(c2) ? 1.0 : -1.0; any = true; }
      }
    }
    if (!any) return e;
    // (scaled as pepsgpu_nn_hop_slice_fermion scales them: the bond energies of the hook are those of the slice, bit for bit)
    const DeviceTraceScaling<TenElemT> scaling(comp.contractor);
    const std::vector<TenElemT> psi = comp.contractor.Trace(s1, orient);
    const std::vector<TenElemT> psi_ex = comp.ReplaceNNSiteTrace(s1, s2, orient, 2, cand);
    for (size_t w = 0; w < n; ++w) {
      const int32_t c1 = comp.config(w, s1), c2 = comp.config(w, s2);
      if (c1 == c2) continue;
      const TenElemT &p = NonZeroPsi(psi[w]);
      e[w] = BondEnergyFromHops(c1, c2, ComplexConjugate(TenElemT(sign[2 * w] * psi_ex[2 * w] / p)),
                                ComplexConjugate(TenElemT(sign[2 * w + 1] * psi_ex[2 * w + 1] / p)));
    }
    return e;
  }
  double EvaluateTotalOnsiteEnergy(const Configuration &config, size_t w) const {   // :101-117
    size_t doublons = 0, electrons = 0;
    for (size_t r = 0; r < config.rows(); ++r)
      for (size_t c = 0; c < config.cols(); ++c) {
        doublons += config(w, {r, c}) == 0;
        electrons += (size_t)HubbardConfig2Density((size_t)config(w, {r, c}));
      }
    return U_ * double(doublons) - mu_ * double(electrons);
  }
  // the registry of the nearest-neighbour form plus the doublon indicator (:127-171)
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {
    std::vector<ObservableMeta> out = SquareNNModelMeasurementSolver<SquareHubbardModel>::DescribeObservables(ly, lx);
    out.push_back({"double_occupancy", "On-site double occupancy indicator (Ly,Lx)", {ly, lx}, {"y", "x"}});
    return out;
  }
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp) {
    ObservableMapT<TenElemT> out = SquareNNModelMeasurementSolver<SquareHubbardModel>::EvaluateObservables(sitps, comp);
    const size_t ly = comp.contractor.rows(), lx = comp.contractor.cols(), n = comp.config.walkers();
    auto &dbl = out.make("double_occupancy", ly * lx);
    for (size_t w = 0; w < n; ++w)
      for (size_t s = 0; s < ly * lx; ++s) dbl[w * ly * lx + s] = comp.config(w, {s / lx, s % lx}) == 0 ? 1.0 : 0.0;
    return out;
  }
 private:
  double t_, U_, mu_;
};

// transverse_field_ising_square_obc.h:28-247
class TransverseFieldIsingSquareOBC {
 public:
  explicit TransverseFieldIsingSquareOBC(double h) : h_(h) {}
  double CalDiagTermEnergy(const Configuration &config, size_t w) const {   // :160-182
    double e = 0;
    for (size_t r = 0; r < config.rows(); r++)
      for (size_t c = 0; c + 1 < config.cols(); c++) e += (config(w, {r, c}) == config(w, {r, c + 1})) ? -1 : 1;
    for (size_t c = 0; c < config.cols(); c++)
      for (size_t r = 0; r + 1 < config.rows(); r++) e += (config(w, {r, c}) == config(w, {r + 1, c})) ? -1 : 1;
    return e;
  }
  template <bool calchols = true, typename TenElemT = double>
  EnergyAndHolesT<TenElemT> CalEnergyAndHoles(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp,
                                              bool holes_on_device = false) {   // :211-247
    const size_t n = comp.config.walkers();
    EnergyAndHolesT<TenElemT> out;
    out.energy.assign(n, TenElemT(0.0));
    // the device slice (holes kept in HBM) when the holes are not wanted on the host
    out.psi_list = RowPass(comp, DeviceSlicesEnabled() && (!calchols || holes_on_device),
                           HoleDest<TenElemT>(calchols, holes_on_device, sitps.slot(), comp, out.holes),
                           [&](size_t, size_t, const std::vector<TenElemT> &ex) {
                             for (size_t w = 0; w < n; ++w) out.energy[w] += ex[w];
                           });
    for (size_t w = 0; w < n; ++w) out.energy[w] += CalDiagTermEnergy(comp.config, w);
    return out;
  }
  // Registry of the model (:60-152): energy, spin_z, sigma_x per site (= -off-diagonal term / h; 0 for h = 0), SzSz_row along the
  // middle row (x0 = lx / 4, i = 1 .. lx / 2).  Same row pass as the energy.  (The oracle form is pinned on the reference's
  // exact-sum measurer numbers at 1e-10, tests/test_oracle_measure.py; the device form runs the same registries in
  // tests/test_gpu_measure.py, real and complex.)
  template <typename TenElemT>
  ObservableMapT<TenElemT> EvaluateObservables(const SplitIndexTPST<TenElemT> &, TPSWaveFunctionComponentT<TenElemT> &comp) {
    const size_t ly = comp.contractor.rows(), lx = comp.contractor.cols(), n = comp.config.walkers(), half = lx / 2, row = ly / 2;
    ObservableMapT<TenElemT> out;
    out.n = n;
    auto &sx = out.make("sigma_x", ly * lx);
    auto &sz = out.make("spin_z", ly * lx);
    auto &en = out.make("energy", 1);
    last_psi_.Fill(n, RowPass(comp, DeviceSlicesEnabled(), HoleDest<TenElemT>(), [&](size_t r, size_t col, const std::vector<TenElemT> &ex) {
      for (size_t w = 0; w < n; ++w) {
        en[w] += ex[w];
        sx[w * ly * lx + r * lx + col] = h_ != 0.0 ? TenElemT(-ex[w] / h_) : TenElemT(0.0);                 // :96
      }
    }));
    if (half > 0) {                                                                                         // :101-110
      auto &szsz = out.make("SzSz_row", half);
      for (size_t w = 0; w < n; ++w) {
        const double sz1 = double(comp.config(w, {row, lx / 4})) - 0.5;
        for (size_t i = 1; i <= half; ++i) szsz[w * half + i - 1] = sz1 * (double(comp.config(w, {row, lx / 4 + i})) - 0.5);
      }
    }
    for (size_t w = 0; w < n; ++w) {
      en[w] += CalDiagTermEnergy(comp.config, w);
      for (size_t r = 0; r < ly; ++r)
        for (size_t cc = 0; cc < lx; ++cc) sz[w * ly * lx + r * lx + cc] = double(comp.config(w, {r, cc})) - 0.5;
    }
    return out;
  }
  PsiSummary EvaluatePsiSummary() const { return last_psi_.As<double>(); }
  template <typename TenElemT> PsiSummaryT<TenElemT> EvaluatePsiSummaryT() const { return last_psi_.As<TenElemT>(); }
  std::vector<ObservableMeta> DescribeObservables(size_t ly, size_t lx) const {                        // :142-149
    return {{"energy", "Total energy (scalar)", {}, {}},
            {"spin_z", "Local spin Sz per site (Ly,Lx)", {ly, lx}, {"y", "x"}},
            {"sigma_x", "Transverse magnetisation per site (Ly,Lx)", {ly, lx}, {"y", "x"}},
            {"SzSz_row", "SzSz correlations along middle row (flat)", {lx / 2}, {"segment"}}};
  }
 private:
  // the row pass of one row on the device: InitBTen, GrowFullBTen(RIGHT, row, 1, true), psi = Trace, per site (PunchHoleStore and)
  // ReplaceOneSiteTrace of the flipped spin + ShiftBTenWindow -- psi [walker], psi_ex [walker][col]
  template <typename TenElemT>
  static void FlipSlice(BMPSContractorT<TenElemT> &c, size_t row, bool holes, std::vector<TenElemT> &psi, std::vector<TenElemT> &psi_ex) {
    static const int32_t flip[2] = {1, 0};
    const size_t n = c.walkers(), cols = c.cols();
    psi.assign(n, TenElemT(0.0));
    psi_ex.assign(n * cols, TenElemT(0.0));
    check_rc(pepsgpu_onsite_slice(c.ctx(), HORIZONTAL, (int)row, holes ? 1 : 0, 1, flip, dptr(psi.data()), dptr(psi_ex.data())), c.ctx());
  }
  // The row pass of the energy and of the registry (the model has no column pass: its bond term is diagonal): on_site(row, col, ex) with
  // ex[w] = -h conj(psi(spin flipped at the site) / psi) (:195-203), in a row behind the hole of the site.  dev_slice: a whole row from
  // ONE FlipSlice; PEPSHOST_NO_DEVICE_SWEEP=1 keeps the per-site ReplaceOneSiteTrace.  Returns psi of every row.
  template <typename TenElemT, class OnSite>
  std::vector<std::vector<TenElemT>> RowPass(TPSWaveFunctionComponentT<TenElemT> &comp, bool dev_slice, const HoleDest<TenElemT> &holes,
                                             OnSite &&on_site) const {
    auto &c = comp.contractor;
    const size_t rows = c.rows(), cols = c.cols(), n = comp.config.walkers();
    std::vector<std::vector<TenElemT>> psi_list;
    c.GenerateBMPSApproach(UP);
    for (size_t row = 0; row < rows; row++) {
      std::vector<TenElemT> psi, row_ex;                  // (device slice: the flipped amplitudes of the whole row, [walker][col])
      if (dev_slice) {
        FlipSlice(c, row, holes.wanted, psi, row_ex);
      } else {
        c.InitBTen(LEFT, row);
        c.GrowFullBTen(RIGHT, row, 1, true);
        psi = c.Trace({row, 0}, HORIZONTAL);
      }
      psi_list.push_back(psi);
      for (size_t col = 0; col < cols; col++) {
        std::vector<TenElemT> psi_ex(n), ex(n);
        if (dev_slice) {
          for (size_t w = 0; w < n; ++w) psi_ex[w] = row_ex[w * cols + col];
        } else {
          holes.Punch(c, {row, col});
          std::vector<int32_t> cand(n);
          for (size_t w = 0; w < n; ++w) cand[w] = 1 - comp.config(w, {row, col});
          psi_ex = c.ReplaceOneSiteTrace({row, col}, HORIZONTAL, 1, cand);
        }
        for (size_t w = 0; w < n; ++w) ex[w] = (-h_) * ComplexConjugate(TenElemT(psi_ex[w] / NonZeroPsi(psi[w])));   // :202
        on_site(row, col, ex);
        if (!dev_slice && col + 1 < cols) c.ShiftBTenWindow(RIGHT);
      }
      if (row + 1 < rows) c.ShiftBMPSWindow(DOWN);
    }
    return psi_list;
  }
  double h_;
  PsiSummaryStore last_psi_;
};

// Accumulators of the evaluators: S_O = sum w O*, S_EO = sum w E_loc* O*, sum w, sum w E_loc
// (exact_summation_energy_evaluator.h:195-245; mc_energy_grad_evaluator.h:245-278 with w = 1).
template <typename TenElemT>
struct GradAccumulatorT {
  SplitIndexTPST<TenElemT> Ostar_sum, ELocConj_Ostar_sum;
  double weight_sum = 0.0, e_loc_sq_sum = 0.0;
  TenElemT e_loc_sum = TenElemT(0.0);
  size_t samples = 0;
  static constexpr size_t kScalars = ElemTraits<TenElemT>::is_complex ? 5 : 4;   // weight, E (re [, im]), |E|^2, samples
  GradAccumulatorT(const SplitIndexTPST<TenElemT> &like)
      : Ostar_sum(like.rows(), like.cols(), like.PhysicalDim(), like.D()),
        ELocConj_Ostar_sum(like.rows(), like.cols(), like.PhysicalDim(), like.D()) {}

  // exact summation: weight |psi|^2, O* increment = psi * Dag(hole)        (exact_summation_energy_evaluator.h:231)
  // Monte Carlo:     weight 1,       O* = conj(1 / psi) * Dag(hole)          (mc_energy_grad_evaluator.h:246, :266)
  // S_EO += conj(E_loc) * increment                                          (:239 / :272);  eh.holes already hold Dag(hole)
  void Accumulate(const TPSWaveFunctionComponentT<TenElemT> &comp, const EnergyAndHolesT<TenElemT> &eh, bool exact_sum) {
    const size_t n = comp.config.walkers(), rows = Ostar_sum.rows(), cols = Ostar_sum.cols(), slot = Ostar_sum.slot();
    for (size_t w = 0; w < n; ++w) {
      // fermions: psi = sigma * Dense_row, d psi / d T''_v = sigma * hole: the derivative of ln psi with respect to the
      // DECORATED component (extended state) uses the plain contraction value; FoldFermionGradient maps it back
      const TenElemT psi = comp.fermion ? comp.amplitude[w] * double(comp.fermion->Sigma(comp.config, w)) : comp.amplitude[w];
      const TenElemT e = eh.energy[w], ec = ComplexConjugate(e);
      const double wt = exact_sum ? AbsSquare(psi) : 1.0;
      const TenElemT f = exact_sum ? psi : ComplexConjugate(TenElemT(TenElemT(1.0) / psi));
      for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) {
          const size_t basis = comp.fermion ? (size_t)comp.fermion->Ext(comp.config, w, {r, c}, ROW_MAJOR)
                                            : (size_t)comp.config(w, {r, c});
          const TenElemT *h = eh.holes.data() + ((w * rows + r) * cols + c) * slot;
          TenElemT *so = Ostar_sum.component(r, c, basis), *seo = ELocConj_Ostar_sum.component(r, c, basis);
          for (size_t k = 0; k < slot; ++k) { const TenElemT v = f * h[k]; so[k] += v; seo[k] += ec * v; }
        }
      weight_sum += wt;
      e_loc_sum += e * wt;
      e_loc_sq_sum += AbsSquare(e) * wt;
      ++samples;
    }
  }
  // Same accumulation with the holes resident on the device (BMPSContractor::PunchHoleStore):
  // the tensor sums stay in HBM until FetchDevice() (the device applies Dag() and the conjugations itself).
  // Fermionic states: the stored holes are those of the row-major decorated network, d psi_dense / d T''; the device is told
  // the extended state of every site in that decoration and the plain contraction value psi_dense = sigma * psi (the
  // walkers themselves may be in the column-major decoration by now).
  void AccumulateDevice(TPSWaveFunctionComponentT<TenElemT> &comp, const EnergyAndHolesT<TenElemT> &eh, bool exact_sum) {
    if (comp.fermion) {
      std::vector<TenElemT> dense(comp.amplitude);
      for (size_t w = 0; w < dense.size(); ++w) dense[w] *= double(comp.fermion->Sigma(comp.config, w));
      const Configuration ext = comp.fermion->ExtConfig(comp.config, ROW_MAJOR);
      comp.contractor.GradAccumulate(dense, eh.energy, exact_sum, std::vector<int32_t>(ext.data(), ext.data() + ext.walkers() * ext.rows() * ext.cols()));
    } else {
      comp.contractor.GradAccumulate(comp.amplitude, eh.energy, exact_sum);
    }
    for (size_t w = 0; w < comp.config.walkers(); ++w) {
      const TenElemT psi = comp.amplitude[w], e = eh.energy[w];
      const double wt = exact_sum ? AbsSquare(psi) : 1.0;
      weight_sum += wt; e_loc_sum += e * wt; e_loc_sq_sum += AbsSquare(e) * wt;
      ++samples;
    }
  }
  void FetchDevice(const BMPSContractorT<TenElemT> &c) {
    std::vector<TenElemT> so, seo;
    c.GradRead(so, seo);
    auto &a = Ostar_sum.flat();
    auto &b = ELocConj_Ostar_sum.flat();
    for (size_t k = 0; k < a.size(); ++k) { a[k] += so[k]; b[k] += seo[k]; }
  }
  // Flat view (doubles; a complex element = an interleaved (re, im) pair) for the cross-rank sum that replaces
  // MPIMeanTensor / MPI_Reduce (statistics_tensor.h:37-79, exact_summation_energy_evaluator.h:252-280): one all-reduce(sum).
  // Layout: S_O, S_EO, weight, E_loc sum (re [, im]), |E_loc|^2 sum, samples.
  std::vector<double> Pack() const {
    const size_t m = Ostar_sum.flat().size() * (ElemTraits<TenElemT>::is_complex ? 2 : 1);
    std::vector<double> v;
    v.reserve(2 * m + kScalars);
    v.insert(v.end(), dptr(Ostar_sum.flat().data()), dptr(Ostar_sum.flat().data()) + m);
    v.insert(v.end(), dptr(ELocConj_Ostar_sum.flat().data()), dptr(ELocConj_Ostar_sum.flat().data()) + m);
    v.push_back(weight_sum);
    v.push_back(std::real(e_loc_sum));
    if (ElemTraits<TenElemT>::is_complex) v.push_back(std::imag(e_loc_sum));
    v.push_back(e_loc_sq_sum); v.push_back((double)samples);
    return v;
  }
  void Unpack(const std::vector<double> &v) {
    const size_t m = Ostar_sum.flat().size() * (ElemTraits<TenElemT>::is_complex ? 2 : 1);
    std::copy(v.begin(), v.begin() + m, dptr(Ostar_sum.flat().data()));
    std::copy(v.begin() + m, v.begin() + 2 * m, dptr(ELocConj_Ostar_sum.flat().data()));
    size_t o = 2 * m;
    weight_sum = v[o++];
    if constexpr (ElemTraits<TenElemT>::is_complex) { e_loc_sum = TenElemT(v[o], v[o + 1]); o += 2; }
    else e_loc_sum = v[o++];
    e_loc_sq_sum = v[o++]; samples = (size_t)v[o++];
  }
  // energy = sum wE / sum w ; gradient = (S_EO - E* S_O) / sum w   (exact_summation_energy_evaluator.h:286-295)
  std::pair<TenElemT, SplitIndexTPST<TenElemT>> Finish() const {
    const TenElemT energy = e_loc_sum / weight_sum, ec = ComplexConjugate(energy);
    SplitIndexTPST<TenElemT> grad(Ostar_sum.rows(), Ostar_sum.cols(), Ostar_sum.PhysicalDim(), Ostar_sum.D());
    const auto &so = Ostar_sum.flat(), &seo = ELocConj_Ostar_sum.flat();
    auto &g = grad.flat();
    for (size_t k = 0; k < g.size(); ++k) g[k] = (seo[k] - ec * so[k]) / weight_sum;
    return {energy, grad};
  }
};
using GradAccumulator = GradAccumulatorT<double>;

// MonteCarloEngine (algorithm/vmc_update/monte_carlo_engine.h): warm-up, sweeps, amplitude sanity, configuration rescue and
// the order-1 normalisation of the state, for a walker batch.  The reference holds one walker per MPI rank; here a Monte-Carlo
// walker of the context takes the place of a rank: EnsureConfigurationValidity (:340-414) replaces the configuration of every
// walker whose construction failed (device flag: empty tensor) or whose amplitude is outside (min, max) by the configuration of
// the first valid walker -- the reference's "first valid rank" -- and marks the batch as not warmed up; NormalizeStateOrder1
// (:206-240) scales every site tensor by (1 / max_w |psi_w|)^(1 / (Lx Ly)) and rebuilds the components.  More ranks: hand a
// max-over-ranks functor (e.g. on BMPSContractor::AllReduceMax); rescue is rank-local (a rank holds thousands of walkers).
struct ConfigurationRescueParams {                 // psi_consistency.h:59-85
  bool enabled = true;
  double amplitude_min_threshold = std::numeric_limits<double>::min();
  double amplitude_max_threshold = std::numeric_limits<double>::max();
};
struct MonteCarloParams {                          // monte_carlo_peps_params.h
  size_t num_warmup_sweeps = 0, sweeps_between_samples = 1;
  bool is_warmed_up = false;
  size_t samples_per_walker = 1;                   // num_samples of a rank (a walker plays the rank): MCEnergyGradEvaluator, VMCPEPSOptimizer
  std::string config_dump_path;                    // VMCPEPSOptimizer::DumpData: configuration<walker> files; empty = no dump
};
template <typename TenElemT>
inline bool CheckWaveFunctionAmplitudeValidity(const TenElemT &amplitude, double min_threshold, double max_threshold) {   // wave_function_component.h:393-402
  const double a = std::abs(amplitude);
  return !std::isnan(a) && !std::isinf(a) && a > min_threshold && a < max_threshold;
}
template <class MonteCarloSweepUpdater, typename TenElemT = double>
class MonteCarloEngine {
 public:
  MonteCarloEngine(SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp, const MonteCarloParams &params,
                   MonteCarloSweepUpdater &updater, const ConfigurationRescueParams &rescue = ConfigurationRescueParams(),
                   std::function<double(double)> max_over_ranks = nullptr,
                   std::function<int(int, int, int32_t *)> exchange_valid_config = nullptr)
      : sitps_(sitps), comp_(comp), params_(params), updater_(updater), rescue_(rescue), max_over_ranks_(std::move(max_over_ranks)),
        exchange_valid_config_(std::move(exchange_valid_config)), warm_up_(params.is_warmed_up) {
    EnsureConfigurationValidity();                 // the constructor's last step (:112-113)
  }
  // Resident mode: the state lives on the device as the master parameters of an Optimizer (pepsgpu_opt_begin) and never crosses PCIe:
  // NormalizeStateOrder1 scales it there (pepsgpu_opt_scale_state).  `shape` gives the extents only (fermions: the 4 d decorated
  // components); `comp` was built on the resident state (TPSWaveFunctionComponentT::ResidentState).  One rank.
  MonteCarloEngine(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState, SplitIndexTPST<TenElemT> &shape,
                   TPSWaveFunctionComponentT<TenElemT> &comp, const MonteCarloParams &params, MonteCarloSweepUpdater &updater,
                   const ConfigurationRescueParams &rescue = ConfigurationRescueParams())
      : sitps_(shape), comp_(comp), params_(params), updater_(updater), rescue_(rescue), warm_up_(params.is_warmed_up), resident_(true) {
    EnsureConfigurationValidity();
  }
  bool IsResident() const { return resident_; }
  TPSWaveFunctionComponentT<TenElemT> &WavefuncComp() { return comp_; }
  const TPSWaveFunctionComponentT<TenElemT> &WavefuncComp() const { return comp_; }
  // the host state; in resident mode the extents only (the tensors are the device's)
  const SplitIndexTPST<TenElemT> &State() const { return sitps_; }
  const MonteCarloParams &Params() const { return params_; }
  // RefreshWavefunctionComponent (monte_carlo_engine.h, used at mc_energy_grad_evaluator.h:164): the walkers' environments are rebuilt on
  // the state the device now holds and the amplitudes are taken afresh; the configurations and the updater's mt19937 engines stay.
  void RefreshWavefunctionComponent() {
    comp_.order = ROW_MAJOR;
    comp_.InitDevice();
    comp_.EvaluateAmplitude();
  }
  bool IsWarmedUp() const { return warm_up_; }
  size_t RescuedWalkers() const { return n_rescued_; }
  double LastScaleFactor() const { return last_scale_; }
  std::vector<double> StepSweep(size_t sweeps) {   // :176-189
    std::vector<double> rates;
    for (size_t i = 0; i < sweeps; ++i) updater_(sitps_, comp_, rates);
    return rates;
  }
  std::vector<double> StepSweep() { return StepSweep(params_.sweeps_between_samples); }
  int WarmUp() {                                   // :146-173
    if (!warm_up_) {
      for (size_t s = 0; s < params_.num_warmup_sweeps; ++s) (void)StepSweep(1);
      warm_up_ = true;
    }
    for (size_t w = 0; w < comp_.amplitude.size(); ++w)
      if (!CheckWaveFunctionAmplitudeValidity(comp_.amplitude[w], rescue_.amplitude_min_threshold, rescue_.amplitude_max_threshold))
        throw std::runtime_error("MonteCarloEngine::WarmUp: amplitude of walker " + std::to_string(w) + " is still not legal after warm up");
    NormalizeStateOrder1();
    return 0;
  }
  void NormalizeStateOrder1() {                    // :206-240
    double max_abs = 0.0;
    for (const auto &a : comp_.amplitude) max_abs = std::max(max_abs, (double)std::abs(a));
    if (max_over_ranks_) max_abs = max_over_ranks_(max_abs);
    if (!(max_abs > 0.0) || std::isinf(max_abs)) throw std::runtime_error("MonteCarloEngine::NormalizeStateOrder1: no finite non-zero amplitude");
    last_scale_ = 1.0 / max_abs;
    const double on_site = std::pow(last_scale_, 1.0 / double(comp_.contractor.rows() * comp_.contractor.cols()));
    if (resident_) {
      comp_.contractor.OptScaleState(on_site);     // theta *= scale_factor_on_site, device state = T(theta): no state crosses PCIe
    } else {
      for (auto &x : sitps_.flat()) x *= on_site;  // split_index_tps_ *= scale_factor_on_site
      comp_.contractor.UploadState(sitps_);        // tps_sample_ = WaveFunctionComponentT(split_index_tps_, config, trun_para)
    }
    comp_.InitDevice();
    comp_.EvaluateAmplitude();
  }
  void EnsureConfigurationValidity() {             // :340-414
    const size_t n = comp_.config.walkers();
    std::vector<int32_t> flags = comp_.contractor.WalkerFlags();
    std::vector<uint8_t> valid(n);
    size_t num_valid = 0;
    for (size_t w = 0; w < n; ++w) {
      valid[w] = !flags[w] && CheckWaveFunctionAmplitudeValidity(comp_.amplitude[w], rescue_.amplitude_min_threshold, rescue_.amplitude_max_threshold);
      num_valid += valid[w];
    }
    // Several ranks (exchange_valid_config_ set): the reference's walkers are its MPI ranks -- MPI_Allgather of the validity flags,
    // the FIRST valid rank broadcasts its configuration (:344-387).  Here the global order is (rank, walker): the callback is the
    // collective (every rank calls it, valid or not): in = number of invalid local walkers, whether this rank holds a valid one and
    // the configuration of its first valid walker; out = that configuration of the lowest rank that holds one; returns the
    // number of invalid walkers over all ranks, -1 when no rank holds a valid one.
    const size_t sites = comp_.config.rows() * comp_.config.cols();
    std::vector<int32_t> donor(sites, 0);
    size_t source = 0;
    while (source < n && !valid[source]) ++source;
    if (source < n)
      for (size_t r = 0; r < comp_.config.rows(); ++r)
        for (size_t c = 0; c < comp_.config.cols(); ++c) donor[r * comp_.config.cols() + c] = (int32_t)comp_.config(source, {r, c});
    long invalid_total = (long)(n - num_valid);
    bool any_valid = num_valid > 0;
    if (exchange_valid_config_) {
      const int tot = exchange_valid_config_((int)(n - num_valid), num_valid > 0 ? 1 : 0, donor.data());
      any_valid = tot >= 0;
      invalid_total = tot;
    }
    if (invalid_total == 0) return;
    if (!rescue_.enabled)
      throw std::runtime_error("MonteCarloEngine: " + std::to_string(invalid_total) +
                               " walkers have invalid configurations and configuration rescue is disabled");
    if (!any_valid)
      throw std::runtime_error("MonteCarloEngine: all walkers have invalid configurations (check bond dimension, truncation cutoff, initial configuration)");
    if (num_valid == n) return;                    // (other ranks rescue theirs)
    Configuration cfg = comp_.config;
    for (size_t w = 0; w < n; ++w)
      if (!valid[w])
        for (size_t r = 0; r < cfg.rows(); ++r)
          for (size_t c = 0; c < cfg.cols(); ++c) cfg(w, {r, c}) = donor[r * cfg.cols() + c];
    comp_.config = cfg;
    comp_.InitDevice();
    flags = comp_.EvaluateAmplitudeNoThrow();      // TryConstructWavefunction_(config_valid)
    for (size_t w = 0; w < n; ++w)
      if (flags[w] || !CheckWaveFunctionAmplitudeValidity(comp_.amplitude[w], rescue_.amplitude_min_threshold, rescue_.amplitude_max_threshold))
        throw std::runtime_error("MonteCarloEngine: rescue FAILED for walker " + std::to_string(w) + " even with a valid configuration" +
                                 (exchange_valid_config_ ? std::string(" of the first valid rank") : " of walker " + std::to_string(source)));
    n_rescued_ += n - num_valid;
    warm_up_ = false;
  }

 private:
  SplitIndexTPST<TenElemT> &sitps_;
  TPSWaveFunctionComponentT<TenElemT> &comp_;
  MonteCarloParams params_;
  MonteCarloSweepUpdater &updater_;
  ConfigurationRescueParams rescue_;
  std::function<double(double)> max_over_ranks_;
  std::function<int(int, int, int32_t *)> exchange_valid_config_;
  bool warm_up_;
  size_t n_rescued_ = 0;
  double last_scale_ = 1.0;
  bool resident_ = false;
};

// GenerateAllPermutationConfigs (exact_summation_energy_evaluator.h:74-95) for one walker batch layout
// MCPEPSMeasurer (algorithm/vmc_update/monte_carlo_peps_measurer{.h,_impl.h}): warm-up, then per sample
// `sweeps_between_samples` Monte-Carlo sweeps + EvaluateObservables + psi summary.  A walker of the batch plays the role
// of an MPI rank of the reference: per-walker sample means (SampleData::StatisticRegistry, monte_carlo_peps_measurer.h:369-396),
// then mean and standard error across the walkers (GatherStatisticListOfData, monte_carlo_tools/statistics.h:289-340;
// ranks of other GPUs are merged by the caller from Partial()).
struct MCMeasurementParams {                       // MonteCarloParams (monte_carlo_peps_params.h)
  size_t num_samples = 1, num_warmup_sweeps = 0, sweeps_between_samples = 1;
  // false: the warm-up is the plain sweeps followed by a fresh amplitude, without NormalizeStateOrder1's rescaling of the state -- the
  // chain and the sampled ratios are then those of a caller that sweeps and evaluates by hand (pepshost_fermion_measure_energy)
  bool normalize_state = true;
};
template <class MonteCarloSweepUpdater, class MeasurementSolver, typename TenElemT = double>
class MCPEPSMeasurer {
 public:
  MCPEPSMeasurer(const SplitIndexTPST<TenElemT> &sitps, TPSWaveFunctionComponentT<TenElemT> &comp, const MCMeasurementParams &params,
                 MonteCarloSweepUpdater &updater, MeasurementSolver &solver)
      : sitps_(sitps), comp_(comp), params_(params), updater_(updater), solver_(solver) {
    observables_meta_ = solver_.DescribeObservables(comp.contractor.rows(), comp.contractor.cols());
  }
  // NOTE on ownership (differs from the reference, where the measurer owns engine and state): the warm-up's NormalizeStateOrder1
  // rescales the measurer's PRIVATE copy of the state and uploads it into the caller's contractor / component; the caller's own
  // SplitIndexTPS is only held by const reference and is NOT rescaled.  After Execute() the device holds State(), which differs from
  // the caller's host state by StateScaleFactor(): keep using State() (or re-upload your own state) with this component afterwards.
  // The engine constructor also runs EnsureConfigurationValidity: invalid walkers throw here instead of being swept.
  void Execute() {                                  // monte_carlo_peps_measurer_impl.h:172-178
    // engine_.WarmUp() (monte_carlo_engine.h:146-173): the warm-up sweeps, the amplitude sanity check and NormalizeStateOrder1 -- the
    // measurer's own copy of the state is rescaled to max_w |psi_w| = 1 and the components are rebuilt.  Ratios do not see it; the
    // structure-factor amplitudes (SpSm_cross) do, and the reference's regression vector (K8) is taken after it.
    if (!params_.normalize_state) {
      std::vector<double> rates;
      for (size_t s = 0; s < params_.num_warmup_sweeps; ++s) updater_(sitps_, comp_, rates);
      comp_.SetOrder(ROW_MAJOR);
      comp_.EvaluateAmplitude();
      Measure_();
      return;
    }
    MonteCarloParams mc;
    mc.num_warmup_sweeps = params_.num_warmup_sweeps;
    mc.sweeps_between_samples = params_.sweeps_between_samples;
    MonteCarloEngine<MonteCarloSweepUpdater, TenElemT> engine(sitps_, comp_, mc, updater_);
    engine.WarmUp();
    scale_factor_ = engine.LastScaleFactor();
    Measure_();
  }
  double StateScaleFactor() const { return scale_factor_; }   // overall factor of NormalizeStateOrder1 (1 / max |psi| after warm-up)
  const SplitIndexTPST<TenElemT> &State() const { return sitps_; }       // the rescaled state the samples were taken on
  // key -> (mean, stderr) over the walkers of this batch; the mean has the element type, the standard error is real (statistics.h:289-340)
  const std::map<std::string, std::pair<std::vector<TenElemT>, std::vector<double>>> &ObservableRegistry() const { return registry_stats_; }
  // per-walker sample means [key][walker][len]: what a rank contributes to GatherStatisticListOfData
  const std::map<std::string, std::vector<TenElemT>> &WalkerMeans() const { return walker_means_; }
  std::pair<TenElemT, double> OutputEnergy() const {  // :676-690
    const auto &e = registry_stats_.at("energy");
    return {e.first[0], e.second.empty() ? 0.0 : e.second[0]};
  }
  const std::vector<double> &AcceptRates() const { return accept_avg_; }
  // energy_samples[sample][walker]: the "energy" key of every sample (empty when the solver reports none)
  const std::vector<std::vector<TenElemT>> &EnergySamples() const { return energy_samples_; }
  // psi_samples[sample][walker] = (psi_mean, psi_rel_err)
  const std::vector<std::vector<std::pair<TenElemT, double>>> &PsiSamples() const { return psi_samples_; }
  // stats/<key>_mean.csv + <key>_stderr.csv for two-dimensional observables, stats/<key>.csv ("index,mean,stderr") otherwise,
  // samples/psi.csv (impl.h:262-345, :544-640)
  void DumpData(const std::string &dir) const {
    const std::string base = dir.empty() ? "./" : dir + "/";
    auto mk = [](const std::string &d) {
      std::string cmd;
      for (size_t k = 1; k <= d.size(); ++k)
        if (k == d.size() || d[k] == '/') ::mkdir(d.substr(0, k).c_str(), 0755);
    };
    mk(base + "stats");
    mk(base + "samples");
    auto csv = [](const auto &val) {                 // (a complex mean is written by its real part, as the reference's DumpVecData)
      const double v = std::real(val);
      std::ostringstream oss;
      oss.setf(std::ios::scientific, std::ios::floatfield);
      oss << std::setprecision(std::numeric_limits<double>::max_digits10) << v;
      return oss.str();
    };
    for (const auto &kv : registry_stats_) {
      const auto &vals = kv.second.first;
      const auto &errs = kv.second.second;
      const ObservableMeta *meta = nullptr;
      for (const auto &m : observables_meta_) if (m.key == kv.first) meta = &m;
      if (meta && meta->shape.size() == 2 && meta->shape[0] * meta->shape[1] == vals.size()) {
        for (int which = 0; which < 2; ++which) {
          std::ofstream ofs(base + "stats/" + kv.first + (which ? "_stderr.csv" : "_mean.csv"));
          for (size_t r = 0; r < meta->shape[0]; ++r) {
            for (size_t c = 0; c < meta->shape[1]; ++c) {
              const size_t idx = r * meta->shape[1] + c;
              ofs << csv(which ? (idx < errs.size() ? errs[idx] : 0.0) : vals[idx]) << (c + 1 < meta->shape[1] ? "," : "");
            }
            ofs << "\n";
          }
        }
      } else {
        std::ofstream ofs(base + "stats/" + kv.first + ".csv");
        ofs << "index,mean,stderr\n";
        for (size_t k = 0; k < vals.size(); ++k) ofs << k << "," << csv(vals[k]) << "," << csv(k < errs.size() ? errs[k] : 0.0) << "\n";
      }
    }
    for (const auto &m : observables_meta_)          // stats/<key>_coords.txt of an observable with a coordinate generator (impl.h:339-345)
      if (m.coord_generator && registry_stats_.count(m.key))
        std::ofstream(base + "stats/" + m.key + "_coords.txt") << m.coord_generator(comp_.contractor.rows(), comp_.contractor.cols());
    std::ofstream ofs(base + "samples/psi.csv");
    ofs << "sample,walker,psi_mean,psi_rel_err\n";
    for (size_t k = 0; k < psi_samples_.size(); ++k)
      for (size_t w = 0; w < psi_samples_[k].size(); ++w)
        ofs << k << "," << w << "," << csv(psi_samples_[k][w].first) << "," << csv(psi_samples_[k][w].second) << "\n";
  }

 private:
  void Measure_() {                                 // impl.h:495-541
    const size_t n = comp_.config.walkers();
    std::vector<double> rates;
    accept_avg_.assign(n, 0.0);
    std::map<std::string, std::vector<TenElemT>> sum;
    for (size_t sample = 0; sample < params_.num_samples; ++sample) {
      std::vector<double> acc(n, 0.0);
      for (size_t k = 0; k < params_.sweeps_between_samples; ++k) {    // engine_.StepSweep()
        updater_(sitps_, comp_, rates);
        for (size_t w = 0; w < n; ++w) acc[w] += rates[w];
      }
      for (size_t w = 0; w < n; ++w) accept_avg_[w] += acc[w] / double(std::max<size_t>(params_.sweeps_between_samples, 1));
      ObservableMapT<TenElemT> obs = solver_.EvaluateObservables(sitps_, comp_);  // MeasureSample_ (:193-238)
      if (obs.values.count("energy")) energy_samples_.push_back(obs.values.at("energy"));
      for (const auto &kv : obs.values) {
        auto &dst = sum[kv.first];
        if (dst.empty()) dst.assign(kv.second.size(), TenElemT(0.0));
        for (size_t k = 0; k < kv.second.size(); ++k) dst[k] += kv.second[k];
      }
      const PsiSummaryT<TenElemT> ps = solver_.template EvaluatePsiSummaryT<TenElemT>();
      std::vector<std::pair<TenElemT, double>> row(n);
      for (size_t w = 0; w < n; ++w) row[w] = {ps.psi_mean[w], ps.psi_rel_err[w]};
      psi_samples_.push_back(row);
    }
    for (auto &a : accept_avg_) a /= double(std::max<size_t>(params_.num_samples, 1));
    // GatherStatistic_ (:242-258): local (walker) means, then mean / standard error across the walkers
    for (auto &kv : sum) {
      for (auto &v : kv.second) v /= double(params_.num_samples);
      const size_t len = kv.second.size() / n;
      std::vector<TenElemT> mean(len, TenElemT(0.0));
      std::vector<double> err;
      for (size_t w = 0; w < n; ++w)
        for (size_t k = 0; k < len; ++k) mean[k] += kv.second[w * len + k];
      for (auto &m : mean) m /= double(n);
      if (n > 1) {                                  // world_size == 1 leaves std_err empty (statistics.h:304-308)
        err.assign(len, 0.0);
        for (size_t k = 0; k < len; ++k) {
          double var = 0.0;
          for (size_t w = 0; w < n; ++w) var += std::norm(kv.second[w * len + k] - mean[k]);
          err[k] = std::sqrt(var / double(n) / (double(n) - 1.0));      // StandardError (:89-96)
        }
      }
      registry_stats_[kv.first] = {mean, err};
      walker_means_[kv.first] = kv.second;
    }
  }
  SplitIndexTPST<TenElemT> sitps_;                  // by value, as the reference's engine holds split_index_tps_: it is rescaled
  double scale_factor_ = 1.0;
  TPSWaveFunctionComponentT<TenElemT> &comp_;
  MCMeasurementParams params_;
  MonteCarloSweepUpdater &updater_;
  MeasurementSolver &solver_;
  std::vector<ObservableMeta> observables_meta_;
  std::map<std::string, std::pair<std::vector<TenElemT>, std::vector<double>>> registry_stats_;
  std::map<std::string, std::vector<TenElemT>> walker_means_;
  std::vector<std::vector<std::pair<TenElemT, double>>> psi_samples_;
  std::vector<std::vector<TenElemT>> energy_samples_;
  std::vector<double> accept_avg_;
};

inline std::vector<std::vector<int32_t>> GenerateAllPermutationConfigs(const std::vector<size_t> &particle_counts, size_t Lx, size_t Ly) {
  std::vector<int32_t> base;
  for (size_t i = 0; i < particle_counts.size(); ++i)
    for (size_t j = 0; j < particle_counts[i]; ++j) base.push_back((int32_t)i);
  (void)Lx; (void)Ly;
  std::vector<std::vector<int32_t>> all;
  do { all.push_back(base); } while (std::next_permutation(base.begin(), base.end()));
  return all;
}

// GenerateAllBinaryConfigs (exact_summation_measurer.h:53-72): bit `b` of the counter is site (b / Lx, b % Lx)
inline std::vector<std::vector<int32_t>> GenerateAllBinaryConfigs(size_t Lx, size_t Ly) {
  if (Ly != 0 && Lx > std::numeric_limits<size_t>::max() / Ly) throw std::invalid_argument("GenerateAllBinaryConfigs: Lx*Ly overflows size_t");
  const size_t N = Lx * Ly;
  if (N >= (size_t)std::numeric_limits<size_t>::digits) throw std::invalid_argument("GenerateAllBinaryConfigs: Lx*Ly must be < size_t bit width");
  std::vector<std::vector<int32_t>> all((size_t)1 << N, std::vector<int32_t>(N));
  for (size_t i = 0; i < all.size(); ++i)
    for (size_t bit = 0; bit < N; ++bit) all[i][bit] = (int32_t)((i >> bit) & 1);
  return all;
}

// ExactSumMeasurerMPI (exact_summation_measurer.h:103-257): <O> = sum_S |psi(S)|^2 O_loc(S) / sum_S |psi(S)|^2 with
// O_loc from the solver's registry (EvaluateObservables).  Configurations i = rank, rank + size, ... of this rank go
// through the device `batch` walkers at a time; `allreduce` sums [weight | key values in sorted key order] over the
// ranks in place (identity if null: the result is then this rank's share, normalised by its own weight).
// QLTEN_Complex: the packed vector carries every value as a (re, im) pair after the (real) weight.
template <typename MeasurementSolverT, typename TenElemT>
std::map<std::string, std::vector<TenElemT>> ExactSumMeasurer(const SplitIndexTPST<TenElemT> &sitps, const std::vector<std::vector<int32_t>> &all_configs,
                                                              BMPSContractorT<TenElemT> &contractor, MeasurementSolverT &solver, int rank, int size,
                                                              size_t batch, const std::function<void(std::vector<double> &)> &allreduce,
                                                              double *weight_sum_out = nullptr, const FermionDecoration *fermion = nullptr) {
  if (all_configs.empty()) throw std::invalid_argument("ExactSumMeasurerMPI: all_configs must not be empty");     // :113-115
  const size_t rows = sitps.rows(), cols = sitps.cols();
  double weight_rank = 0.0;
  std::map<std::string, std::vector<TenElemT>> weighted;        // std::map: keys already in the sorted order of :153-171
  std::vector<size_t> mine;
  for (size_t i = rank; i < all_configs.size(); i += size) mine.push_back(i);                                     // :130
  // the packed layout comes from the keys this rank evaluated (the reference broadcasts the master's, :173-206)
  // decided from (size, count) alone, i.e. identically on every rank BEFORE any collective: a rank-divergent throw
  // would leave the other ranks waiting in the all-reduce
  if ((size_t)size > all_configs.size() && allreduce) throw std::invalid_argument("ExactSumMeasurer: more ranks than configurations");
  contractor.UploadState(sitps);
  for (size_t b0 = 0; b0 < mine.size(); b0 += batch) {
    const size_t nb = std::min(batch, mine.size() - b0);
    Configuration cfg(nb, rows, cols);
    for (size_t w = 0; w < nb; ++w) std::copy(all_configs[mine[b0 + w]].begin(), all_configs[mine[b0 + w]].end(), cfg.data() + w * rows * cols);
    TPSWaveFunctionComponentT<TenElemT> comp(sitps, cfg, contractor, fermion);
    const std::vector<TenElemT> psi = comp.amplitude;          // the solver's passes may touch comp
    ObservableMapT<TenElemT> obs = solver.EvaluateObservables(sitps, comp);
    for (size_t w = 0; w < nb; ++w) weight_rank += std::norm(psi[w]);                                              // :135-136
    for (const auto &kv : obs.values) {
      const size_t len = kv.second.size() / nb;
      auto &acc = weighted[kv.first];
      if (acc.empty()) acc.assign(len, TenElemT(0.0));
      for (size_t w = 0; w < nb; ++w)
        for (size_t j = 0; j < len; ++j) acc[j] += std::norm(psi[w]) * kv.second[w * len + j];                     // :141-149
    }
  }
  constexpr size_t z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  std::vector<double> packed{weight_rank};
  for (const auto &kv : weighted) packed.insert(packed.end(), dptr(kv.second.data()), dptr(kv.second.data()) + z * kv.second.size());
  if (allreduce) allreduce(packed);                                                                                // :209-235
  const double weight_sum = packed[0];
  if (weight_sum_out) *weight_sum_out = weight_sum;
  if (!(weight_sum > 0.0)) throw std::runtime_error("ExactSumMeasurerMPI: total weight must be positive");         // :243-245
  size_t off = 1;
  for (auto &kv : weighted)
    for (auto &v : kv.second) {                                                                                    // :246-250
      if constexpr (z == 2) v = TenElemT(packed[off], packed[off + 1]) / weight_sum; else v = packed[off] / weight_sum;
      off += z;
    }
  return weighted;
}

// ExactSumEnergyEvaluatorMPI (exact_summation_energy_evaluator.h:173-302): configurations
// i = rank, rank + size, ... are evaluated in batches of `batch` walkers; `allreduce` sums the
// packed accumulators over ranks in place (RCCL all-reduce in the host program; identity if null).
template <typename ModelT, typename TenElemT>
std::pair<TenElemT, SplitIndexTPST<TenElemT>> ExactSumEnergyEvaluator(const SplitIndexTPST<TenElemT> &sitps,
                                                                      const std::vector<std::vector<int32_t>> &all_configs,
                                                                      BMPSContractorT<TenElemT> &contractor, ModelT &model, int rank, int size,
                                                                      size_t batch, const std::function<void(std::vector<double> &)> &allreduce,
                                                                      const FermionDecoration *fermion = nullptr) {
  const size_t rows = sitps.rows(), cols = sitps.cols();
  GradAccumulatorT<TenElemT> acc(sitps);
  std::vector<size_t> mine;
  for (size_t i = rank; i < all_configs.size(); i += size) mine.push_back(i);                 // :201
  contractor.UploadState(sitps);
  contractor.GradReset();
  for (size_t b0 = 0; b0 < mine.size(); b0 += batch) {
    const size_t nb = std::min(batch, mine.size() - b0);
    Configuration cfg(nb, rows, cols);
    for (size_t w = 0; w < nb; ++w) std::copy(all_configs[mine[b0 + w]].begin(), all_configs[mine[b0 + w]].end(), cfg.data() + w * rows * cols);
    TPSWaveFunctionComponentT<TenElemT> comp(sitps, cfg, contractor, fermion);
    // (fermions: the gradient is taken with respect to the decorated -- extended -- components; FoldFermionGradient maps it back)
    EnergyAndHolesT<TenElemT> eh = model.template CalEnergyAndHoles<true>(sitps, comp, /*holes_on_device=*/true);
    acc.AccumulateDevice(comp, eh, true);
  }
  // a contractor with a communicator (CommInit) sums the tensor accumulators over the ranks where they live, in HBM
  // (one RCCL all-reduce each, no host hop), and only the four scalars travel through the host; otherwise the packed
  // host vector goes through the caller's `allreduce` as before
  const bool dev_reduce = contractor.CommSize() > 1;
  if (dev_reduce) contractor.GradAllReduce();
  if (!mine.empty() || dev_reduce) acc.FetchDevice(contractor);
  if (dev_reduce) {
    std::vector<double> sc{acc.weight_sum, std::real(acc.e_loc_sum), std::imag(acc.e_loc_sum), acc.e_loc_sq_sum, (double)acc.samples};
    contractor.AllReduceSum(sc);
    acc.weight_sum = sc[0]; acc.e_loc_sq_sum = sc[3]; acc.samples = (size_t)sc[4];
    if constexpr (ElemTraits<TenElemT>::is_complex) acc.e_loc_sum = TenElemT(sc[1], sc[2]); else acc.e_loc_sum = sc[1];
    return acc.Finish();
  }
  std::vector<double> packed = acc.Pack();
  if (allreduce) allreduce(packed);
  acc.Unpack(packed);
  return acc.Finish();
}

// ---------------------------------------------------------------------------------------------
// Optimizer (optimizer/optimizer.h, optimizer_impl.h) on device buffers: the master parameters, the gradient and the rule
// state live in HBM (pepsgpu_opt_*); an iteration is evaluate -> finish -> clip (first-order rules) -> [natural gradient] ->
// step with no tensor traffic over PCIe.  In: SGD, AdaGrad, Adam and the one-rank SR step, for bosonic and for fermionic states (a
// FermionDecoration with bond parities: the buffers hold the 4 d decorated components, gradients are folded and projected on the
// device, norms and the SR solve are those of the stored parameters); the one-rank MinSR step (MinSRParams: T matrix, eigensolve,
// cutoff and back-substitution on the device, pepsgpu_minsr_direction) for bosonic states; L-BFGS (LBFGSParams) with the fixed step or
// the strong-Wolfe line search for bosonic and fermionic states: history, anchor, direction and the base of the search in HBM
// (pepsgpu_lbfgs_*), every trial point one element-wise pass, one evaluation of the resident state and one dot product; spike
// recovery (S1-S4 with resampling and rollback), the initial and the periodic step selector and checkpoints, with the base of a step,
// the selector trials and the restored state formed in HBM (pepsgpu_guard_*).  Out (host drivers of the reference that stay with
// the caller): the L-BFGS ring snapshot for a rollback, the JSONL log, MinSR over several ranks or on a fermionic state (peps_amd/sr.py), multi-rank CG and the multi-rank broadcast of the
// L-BFGS direction.  Parameter names and defaults: optimizer/optimizer_params.h.
struct ConjugateGradientParams {               // optimizer_params.h:50-57
  size_t max_iter = 100;
  double relative_tolerance = 1e-4;
  double absolute_tolerance = 0.0;
  int residual_recompute_interval = 20;
  double orthogonality_threshold = 0.5;
};
struct SGDParams {                             // :69-76
  double momentum;
  bool nesterov;
  double weight_decay;
  SGDParams(double momentum = 0.0, bool nesterov = false, double weight_decay = 0.0)
      : momentum(momentum), nesterov(nesterov), weight_decay(weight_decay) {}
};
struct AdamParams {                            // :82-90
  double beta1, beta2, epsilon, weight_decay;
  AdamParams(double b1 = 0.9, double b2 = 0.999, double eps = 1e-8, double wd = 0.0) : beta1(b1), beta2(b2), epsilon(eps), weight_decay(wd) {}
};
struct StochasticReconfigurationParams {       // :98-104 (adaptive_diagonal_shift is carried, not applied: the reference does not read it either)
  ConjugateGradientParams cg_params;
  double diag_shift = 0.001;
  bool normalize_update = false;
  double adaptive_diagonal_shift = 0.0;
};
struct AdaGradParams {                         // :192-198
  double epsilon;
  double initial_accumulator_value;
  AdaGradParams(double epsilon, double initial_accumulator_value) : epsilon(epsilon), initial_accumulator_value(initial_accumulator_value) {}
};

class LearningRateScheduler {                  // lr_schedulers.h:29-37
 public:
  virtual ~LearningRateScheduler() = default;
  virtual double GetLearningRate(size_t iteration, double current_energy = 0.0) const = 0;
  virtual void Step() {}
  virtual std::unique_ptr<LearningRateScheduler> Clone() const = 0;
  virtual std::string Name() const = 0;
};
class ConstantLR : public LearningRateScheduler {           // :40-55
 public:
  explicit ConstantLR(double lr) : learning_rate_(lr) {}
  double GetLearningRate(size_t, double) const override { return learning_rate_; }
  std::unique_ptr<LearningRateScheduler> Clone() const override { return std::make_unique<ConstantLR>(learning_rate_); }
  std::string Name() const override { return "ConstantLR"; }
 private:
  double learning_rate_;
};
class ExponentialDecayLR : public LearningRateScheduler {   // :58-80: lr = initial_lr * decay_rate^(iteration / decay_steps)
 public:
  ExponentialDecayLR(double initial_lr, double decay_rate, size_t decay_steps)
      : initial_lr_(initial_lr), decay_rate_(decay_rate), decay_steps_(decay_steps) {}
  double GetLearningRate(size_t iteration, double) const override {
    return initial_lr_ * std::pow(decay_rate_, iteration / static_cast<double>(decay_steps_));
  }
  std::unique_ptr<LearningRateScheduler> Clone() const override { return std::make_unique<ExponentialDecayLR>(initial_lr_, decay_rate_, decay_steps_); }
  std::string Name() const override { return "ExponentialDecayLR"; }
 private:
  double initial_lr_, decay_rate_;
  size_t decay_steps_;
};
class StepLR : public LearningRateScheduler {               // :83-105: lr = initial_lr * gamma^floor(iteration / step_size)
 public:
  StepLR(double initial_lr, size_t step_size, double gamma = 0.1) : initial_lr_(initial_lr), gamma_(gamma), step_size_(step_size) {}
  double GetLearningRate(size_t iteration, double) const override { return initial_lr_ * std::pow(gamma_, iteration / step_size_); }
  std::unique_ptr<LearningRateScheduler> Clone() const override { return std::make_unique<StepLR>(initial_lr_, step_size_, gamma_); }
  std::string Name() const override { return "StepLR"; }
 private:
  double initial_lr_, gamma_;
  size_t step_size_;
};

enum class MinSRSolverMode { kAuto, kReplicated, kDistributed };   // :204-208
struct MinSRParams {                           // :220-232
  double r_pinv, a_pinv;                       // cutoff = r_pinv * max|lambda| + a_pinv
  bool soft_cutoff;                            // lambda^5 / (lambda^6 + cutoff^6) instead of 1 / lambda above the cutoff
  MinSRSolverMode solver_mode;                 // carried, not read: one rank solves on its own device (pepsgpu_minsr_direction)
  MinSRParams(double r_pinv = 1e-12, double a_pinv = 0.0, bool soft_cutoff = true, MinSRSolverMode solver_mode = MinSRSolverMode::kAuto)
      : r_pinv(r_pinv), a_pinv(a_pinv), soft_cutoff(soft_cutoff), solver_mode(solver_mode) {}
};

enum class LBFGSStepMode { kFixed = 0, kStrongWolfe = 1 };   // :110-113
struct LBFGSParams {                           // :119-152
  size_t history_size;                         // pairs kept, 1..32 on the device
  double tolerance_grad;                       // absolute floor for |phi'(alpha)| in the strong-Wolfe curvature test
  double tolerance_change;                     // interval / step tolerance of the line search
  size_t max_eval;                             // evaluations per line search
  LBFGSStepMode step_mode;
  double wolfe_c1, wolfe_c2;                   // 0 < c1 < c2 < 1
  double min_step, max_step;
  double min_curvature;                        // smallest Re<s,y> of an accepted pair
  bool use_damping;
  double max_direction_norm;                   // cap of |d|; <= 0: off
  bool allow_fallback_to_fixed_step;           // a failed search takes max(min_step, lr * fallback_fixed_step_scale) instead of throwing
  double fallback_fixed_step_scale;
  LBFGSParams(size_t hist = 10, double tol_grad = 1e-5, double tol_change = 1e-9, size_t max_eval = 20,
              LBFGSStepMode step_mode = LBFGSStepMode::kFixed, double wolfe_c1 = 1e-4, double wolfe_c2 = 0.9, double min_step = 1e-8,
              double max_step = 1.0, double min_curvature = 1e-12, bool use_damping = true, double max_direction_norm = 1e3,
              bool allow_fallback_to_fixed_step = false, double fallback_fixed_step_scale = 0.2)
      : history_size(hist), tolerance_grad(tol_grad), tolerance_change(tol_change), max_eval(max_eval), step_mode(step_mode),
        wolfe_c1(wolfe_c1), wolfe_c2(wolfe_c2), min_step(min_step), max_step(max_step), min_curvature(min_curvature),
        use_damping(use_damping), max_direction_norm(max_direction_norm), allow_fallback_to_fixed_step(allow_fallback_to_fixed_step),
        fallback_fixed_step_scale(fallback_fixed_step_scale) {}
};

// ---- step selectors, checkpoints and spike recovery: names and defaults of optimizer_params.h:155-313 ----
struct PeriodicStepSelectorParams {            // :164-169
  bool enabled = false;
  size_t every_n_steps = 10;                   // trials at iterations k * every_n_steps, k >= 1
  double phase_switch_ratio = 0.3;             // early / late rule boundary as a fraction of max_iterations
  bool enable_in_deterministic = false;        // run although the evaluator reports no error bar
};
struct InitialStepSelectorParams {             // :180-184
  bool enabled = false;
  size_t max_line_search_steps = 3;            // candidates lr * 1 .. lr * max_line_search_steps at iteration 0
  bool enable_in_deterministic = false;
};
struct CheckpointParams {                      // :278-283
  size_t every_n_steps = 0;                    // 0: off
  std::string base_path;                       // base_path/step_{k}/
  bool IsEnabled() const { return every_n_steps > 0 && !base_path.empty(); }
};
struct SpikeRecoveryParams {                   // :299-313
  bool enable_auto_recover = true;             // S1-S3: evaluate again
  size_t redo_mc_max_retries = 2;              // evaluations repeated per iteration before the last resort
  double factor_err = 100.0;                   // S1: error > factor_err * EMA(error)
  double factor_grad = 1e10;                   // S2: |g| > factor_grad * EMA(|g|)
  double factor_ngrad = 10.0;                  // S3: |x| > factor_ngrad * EMA(|x|), x the natural-gradient direction
  size_t sr_min_iters_suspicious = 1;          // S3: a CG solve of at most this many iterations
  bool enable_rollback = false;                // S4 and the rollback after exhausted retries
  size_t ema_window = 50;
  double sigma_k = 10.0;                       // S4: E - EMA(E) > sigma_k * EMA_std(E)
  std::string log_trigger_csv_path;            // empty: no CSV
};

// ---- spike detection (optimizer/spike_detection.h) ----
enum class SpikeSignal { kNone, kS1_ErrorbarSpike, kS2_GradientNormSpike, kS3_NaturalGradientAnomaly, kS4_EMAEnergySpikeUpward };   // :29-35
enum class SpikeAction { kAccept, kResample, kRollback, kAcceptWithWarning };                                                        // :40-45
struct SpikeEventRecord {                      // :50-57
  size_t step, attempt;
  SpikeSignal signal;
  SpikeAction action;
  double value, threshold;
};
struct SpikeStatistics {                       // :62-67
  size_t total_resamples = 0, total_rollbacks = 0, total_forced_accepts = 0;
  std::vector<SpikeEventRecord> event_log;
};
// exponential moving average with a variance estimate (:80-114): alpha = 2 / (window + 1); the first observation sets the mean and
// var = 0; then delta = x - mean, mean += alpha delta, var = (1 - alpha) (var + alpha delta^2)
class EMATracker {
 public:
  explicit EMATracker(size_t window = 50) : alpha_(2.0 / (static_cast<double>(window) + 1.0)) {}
  void Update(double x) {
    if (!initialized_) { ema_ = x; var_ = 0.0; initialized_ = true; return; }
    const double delta = x - ema_;
    ema_ += alpha_ * delta;
    var_ = (1.0 - alpha_) * (var_ + alpha_ * delta * delta);
  }
  double Mean() const { return ema_; }
  double Var() const { return var_; }
  double Std() const { return std::sqrt(var_); }
  bool IsInitialized() const { return initialized_; }
  void Reset() { ema_ = 0.0; var_ = 0.0; initialized_ = false; }
 private:
  double alpha_, ema_ = 0.0, var_ = 0.0;
  bool initialized_ = false;
};
inline const char *SignalName(SpikeSignal s) {   // :116-125
  switch (s) {
    case SpikeSignal::kNone: return "NONE";
    case SpikeSignal::kS1_ErrorbarSpike: return "S1_ERRORBAR";
    case SpikeSignal::kS2_GradientNormSpike: return "S2_GRAD_NORM";
    case SpikeSignal::kS3_NaturalGradientAnomaly: return "S3_NGRAD_ANOMALY";
    case SpikeSignal::kS4_EMAEnergySpikeUpward: return "S4_ENERGY_SPIKE";
  }
  return "UNKNOWN";
}
inline const char *ActionName(SpikeAction a) {   // :127-135
  switch (a) {
    case SpikeAction::kAccept: return "ACCEPT";
    case SpikeAction::kResample: return "RESAMPLE";
    case SpikeAction::kRollback: return "ROLLBACK";
    case SpikeAction::kAcceptWithWarning: return "ACCEPT_WARN";
  }
  return "UNKNOWN";
}

// The host side of spike recovery, with no device call in it: the four trackers, detection (DetectS1S2_ / DetectS3_ / DetectS4_,
// optimizer_impl.h:1871-1919), the decision (DecideAction_, :1921-1944), the event log and its counters (LogSpikeEvent_, :1955-1973)
// and the trigger CSV (:1841-1856).  Optimizer::IterativeOptimize drives it with device results and acts on the verdicts (evaluate
// again; restore the base); pepshost_spike_replay drives the same object with a scripted series.  "A base is saved" is tracked here
// because the decision reads it (has_prev_state_).
class SpikeGuard {
 public:
  explicit SpikeGuard(const SpikeRecoveryParams &cfg, bool log_to_stdout = true)
      : cfg_(cfg), ema_energy_(cfg.ema_window), ema_error_(cfg.ema_window), ema_grad_norm_(cfg.ema_window), ema_ngrad_norm_(cfg.ema_window),
        log_to_stdout_(log_to_stdout) {}
  SpikeSignal DetectS1S2(double error, double grad_norm) const {
    if (ema_error_.IsInitialized() && ema_error_.Mean() > 0.0 && error > cfg_.factor_err * ema_error_.Mean())
      return SpikeSignal::kS1_ErrorbarSpike;
    if (ema_grad_norm_.IsInitialized() && ema_grad_norm_.Mean() > 0.0 && grad_norm > cfg_.factor_grad * ema_grad_norm_.Mean())
      return SpikeSignal::kS2_GradientNormSpike;
    return SpikeSignal::kNone;
  }
  // a solve that ends within sr_min_iters_suspicious iterations is a signal on its own; MinSR passes SIZE_MAX
  SpikeSignal DetectS3(double ngrad_norm, size_t sr_iters) const {
    if (ema_ngrad_norm_.IsInitialized() && ema_ngrad_norm_.Mean() > 0.0 && ngrad_norm > cfg_.factor_ngrad * ema_ngrad_norm_.Mean())
      return SpikeSignal::kS3_NaturalGradientAnomaly;
    if (sr_iters <= cfg_.sr_min_iters_suspicious) return SpikeSignal::kS3_NaturalGradientAnomaly;
    return SpikeSignal::kNone;
  }
  // upward only, and only once the energies have a spread
  SpikeSignal DetectS4(double energy) const {
    if (!ema_energy_.IsInitialized()) return SpikeSignal::kNone;
    const double delta = energy - ema_energy_.Mean();
    if (delta > 0.0 && ema_energy_.Std() > 0.0 && delta > cfg_.sigma_k * ema_energy_.Std()) return SpikeSignal::kS4_EMAEnergySpikeUpward;
    return SpikeSignal::kNone;
  }
  SpikeAction DecideAction(SpikeSignal signal, size_t attempts, size_t step) const {
    if (signal == SpikeSignal::kNone) return SpikeAction::kAccept;
    if (signal == SpikeSignal::kS4_EMAEnergySpikeUpward) return SpikeAction::kRollback;
    if (attempts < cfg_.redo_mc_max_retries) return SpikeAction::kResample;
    if (cfg_.enable_rollback && has_base_ && step > 0) return SpikeAction::kRollback;
    return SpikeAction::kAcceptWithWarning;
  }
  void LogSpikeEvent(size_t step, size_t attempt, SpikeSignal signal, SpikeAction action, double value, double threshold) {
    if (log_to_stdout_) {
      std::ostringstream os;
      os << "[SPIKE] Step " << step << " attempt " << attempt << " | " << SignalName(signal) << " | value=" << std::scientific
         << std::setprecision(3) << value << " threshold=" << threshold << " | -> " << ActionName(action);
      std::cout << os.str() << std::endl;
    }
    if (action == SpikeAction::kResample) ++stats_.total_resamples;
    else if (action == SpikeAction::kRollback) ++stats_.total_rollbacks;
    else if (action == SpikeAction::kAcceptWithWarning) ++stats_.total_forced_accepts;
    stats_.event_log.push_back({step, attempt, signal, action, value, threshold});
  }
  // The three stages of one evaluation, in the order of optimizer_impl.h:251-297, 683-729, 731-763: detect, decide, log.  The caller
  // evaluates again on kResample (attempts + 1) and on kRollback (after TakeBase, attempts = 0), and goes on otherwise.
  SpikeAction JudgeEvaluation(size_t step, size_t attempts, double error, double grad_norm) {
    if (!cfg_.enable_auto_recover || step == 0) return SpikeAction::kAccept;
    const SpikeSignal signal = DetectS1S2(error, grad_norm);
    if (signal == SpikeSignal::kNone) return SpikeAction::kAccept;
    const SpikeAction action = DecideAction(signal, attempts, step);
    const bool s1 = signal == SpikeSignal::kS1_ErrorbarSpike;
    LogSpikeEvent(step, attempts, signal, action, s1 ? error : grad_norm,
                  s1 ? cfg_.factor_err * ema_error_.Mean() : cfg_.factor_grad * ema_grad_norm_.Mean());
    return action;
  }
  SpikeAction JudgeDirection(size_t step, size_t attempts, double ngrad_norm, size_t sr_iters) {
    if (!cfg_.enable_auto_recover || step == 0) return SpikeAction::kAccept;
    const SpikeSignal signal = DetectS3(ngrad_norm, sr_iters);
    if (signal == SpikeSignal::kNone) return SpikeAction::kAccept;
    const SpikeAction action = DecideAction(signal, attempts, step);
    LogSpikeEvent(step, attempts, signal, action, ngrad_norm, cfg_.factor_ngrad * ema_ngrad_norm_.Mean());
    return action;
  }
  SpikeAction JudgeEnergy(size_t step, size_t attempts, double energy) {
    if (!cfg_.enable_rollback || step == 0) return SpikeAction::kAccept;
    const SpikeSignal signal = DetectS4(energy);
    if (signal == SpikeSignal::kNone) return SpikeAction::kAccept;
    LogSpikeEvent(step, attempts, signal, SpikeAction::kRollback, energy, ema_energy_.Mean() + cfg_.sigma_k * ema_energy_.Std());
    return SpikeAction::kRollback;
  }
  // an accepted evaluation: the only thing the trackers ever see (:765-774)
  void Accept(double energy, double error, double grad_norm, const double *ngrad_norm) {
    ema_energy_.Update(energy);
    ema_error_.Update(error);
    ema_grad_norm_.Update(grad_norm);
    if (ngrad_norm) ema_ngrad_norm_.Update(*ngrad_norm);
  }
  void MarkBaseSaved() { has_base_ = true; }
  // a rollback consumes the base (has_prev_state_ = false): true when there was one to restore
  bool TakeBase() { const bool had = has_base_; has_base_ = false; return had; }
  bool HasBase() const { return has_base_; }
  const SpikeRecoveryParams &Params() const { return cfg_; }
  const SpikeStatistics &Statistics() const { return stats_; }
  const EMATracker &EnergyEMA() const { return ema_energy_; }
  const EMATracker &ErrorEMA() const { return ema_error_; }
  const EMATracker &GradNormEMA() const { return ema_grad_norm_; }
  const EMATracker &NaturalGradNormEMA() const { return ema_ngrad_norm_; }
  static void WriteTriggerCsv(std::ostream &csv, const SpikeStatistics &stats) {
    csv << "step,attempt,signal,action,value,threshold\n";
    for (const auto &ev : stats.event_log)
      csv << ev.step << "," << ev.attempt << "," << SignalName(ev.signal) << "," << ActionName(ev.action) << "," << std::scientific
          << std::setprecision(6) << ev.value << "," << ev.threshold << "\n";
  }
  // nothing is written when no event was logged, as in the reference
  void WriteTriggerCsvFile() const {
    if (cfg_.log_trigger_csv_path.empty() || stats_.event_log.empty()) return;
    std::ofstream csv(cfg_.log_trigger_csv_path);
    if (csv) WriteTriggerCsv(csv, stats_);
  }
 private:
  SpikeRecoveryParams cfg_;
  EMATracker ema_energy_, ema_error_, ema_grad_norm_, ema_ngrad_norm_;
  SpikeStatistics stats_;
  bool has_base_ = false;
  bool log_to_stdout_;
};

// ---- the selection rules of the step selectors (optimizer_impl.h:489-538), with no device call in them ----
struct StepCandidateResult { double eta, energy, error; };
constexpr double kSelectorLateSigma = 1.0;
// the lowest trial energy; the first of equal ones
inline double SelectInitialStep(const std::vector<StepCandidateResult> &r) {
  double selected = r.front().eta, best = r.front().energy;
  for (const auto &c : r)
    if (c.energy < best) { best = c.energy; selected = c.eta; }
  return selected;
}
// r = {eta, eta / 2}.  Early phase (iter < phase_switch_ratio * max_iterations): the half step when its energy is lower at all;
// late phase: only when it is lower by more than kSelectorLateSigma * max(error_eta, error_half)
inline double SelectPeriodicStep(const std::vector<StepCandidateResult> &r, size_t iter, size_t max_iterations, double phase_switch_ratio) {
  const bool early = static_cast<double>(iter) < phase_switch_ratio * static_cast<double>(max_iterations);
  if (early) return r[1].energy < r[0].energy ? r[1].eta : r[0].eta;
  return r[0].energy - r[1].energy > kSelectorLateSigma * std::max(r[0].error, r[1].error) ? r[1].eta : r[0].eta;
}
inline std::vector<double> StepCandidates(bool initial, double base_lr, size_t max_line_search_steps) {
  std::vector<double> etas;
  if (initial) {
    for (size_t i = 1; i <= max_line_search_steps; ++i) etas.push_back(base_lr * static_cast<double>(i));
  } else {
    if (base_lr * 0.5 <= 0.0) throw std::invalid_argument("Auto step selector requires positive candidate step sizes");
    etas = {base_lr, base_lr * 0.5};
  }
  return etas;
}
// the selector's base learning rate after a selection: the initial selector sets it, the periodic one never raises it
inline double NextSelectorBaseLR(bool initial, double base_lr, double selected_eta) {
  return initial ? selected_eta : std::min(base_lr, selected_eta);
}
// a trial's energy and error must be finite (:391-418)
inline void CheckStepCandidate(double energy, double error) {
  const bool bad_e = !std::isfinite(energy), bad_err = !std::isfinite(error);
  if (bad_e && bad_err) throw std::runtime_error("Step selector candidate evaluation produced non-finite energy and energy error");
  if (bad_e) throw std::runtime_error("Step selector candidate evaluation produced non-finite energy");
  if (bad_err) throw std::runtime_error("Step selector candidate evaluation produced non-finite energy error");
}

// (MinSRParams, then LBFGSParams, were appended: the others keep their indices)
using AlgorithmParams = std::variant<SGDParams, AdamParams, StochasticReconfigurationParams, AdaGradParams, MinSRParams, LBFGSParams>;

struct OptimizerParams {                       // optimizer_params.h:348-473
  struct BaseParams {                          // :365-425
    size_t max_iterations;
    double energy_tolerance;
    double gradient_tolerance;
    size_t plateau_patience;
    double learning_rate;
    std::unique_ptr<LearningRateScheduler> lr_scheduler;
    std::optional<double> clip_value;          // per-element magnitude clip, first-order rules only; unset / <= 0: off
    std::optional<double> clip_norm;           // global L2 norm clip, first-order rules only; unset / <= 0: off
    InitialStepSelectorParams initial_step_selector;     // off by default
    PeriodicStepSelectorParams periodic_step_selector;   // off by default
    BaseParams(size_t max_iter, double energy_tol, double grad_tol, size_t patience, double learning_rate,
               std::unique_ptr<LearningRateScheduler> scheduler = nullptr)
        : max_iterations(max_iter), energy_tolerance(energy_tol), gradient_tolerance(grad_tol), plateau_patience(patience),
          learning_rate(learning_rate), lr_scheduler(std::move(scheduler)) {}
    BaseParams(const BaseParams &o)
        : max_iterations(o.max_iterations), energy_tolerance(o.energy_tolerance), gradient_tolerance(o.gradient_tolerance),
          plateau_patience(o.plateau_patience), learning_rate(o.learning_rate),
          lr_scheduler(o.lr_scheduler ? o.lr_scheduler->Clone() : nullptr), clip_value(o.clip_value), clip_norm(o.clip_norm),
          initial_step_selector(o.initial_step_selector), periodic_step_selector(o.periodic_step_selector) {}
    BaseParams &operator=(const BaseParams &o) {
      if (this != &o) { BaseParams t(o); *this = std::move(t); }
      return *this;
    }
    BaseParams(BaseParams &&) = default;
    BaseParams &operator=(BaseParams &&) = default;
  };
  BaseParams base_params;
  AlgorithmParams algorithm_params;
  CheckpointParams checkpoint_params;          // off by default
  SpikeRecoveryParams spike_recovery_params;
  // Deviation from the reference: this constructor switches enable_auto_recover OFF (there S1-S3 stay on).  Runs written against this
  // tree before spike recovery existed must not change, and an SR solve that ends in <= 1 CG iteration is an S3 signal.  The
  // four-argument constructor takes the SpikeRecoveryParams as given; a default-constructed one has the reference's defaults.
  OptimizerParams(const BaseParams &base, const AlgorithmParams &algo) : base_params(base), algorithm_params(algo) {
    spike_recovery_params.enable_auto_recover = false;
  }
  OptimizerParams(const BaseParams &base, const AlgorithmParams &algo, const CheckpointParams &ckpt, const SpikeRecoveryParams &spike)
      : base_params(base), algorithm_params(algo), checkpoint_params(ckpt), spike_recovery_params(spike) {}
  // Every refusal that needs no device (optimizer_impl.h:149-175, and L-BFGS with rollback: the ring snapshot is not built)
  void ValidateGuards() const {
    const bool initial = base_params.initial_step_selector.enabled, periodic = base_params.periodic_step_selector.enabled;
    if (initial || periodic) {
      if (!(IsAlgorithm<SGDParams>() || IsAlgorithm<StochasticReconfigurationParams>() || IsAlgorithm<MinSRParams>()))
        throw std::invalid_argument("Step selectors only support SGD, SR, and MinSR in IterativeOptimize");
      if (base_params.lr_scheduler) throw std::invalid_argument("Step selectors cannot be used together with lr_scheduler in v1");
    }
    if (initial && base_params.initial_step_selector.max_line_search_steps == 0)
      throw std::invalid_argument("Initial step selector max_line_search_steps must be > 0");
    if (periodic) {
      if (base_params.periodic_step_selector.every_n_steps == 0) throw std::invalid_argument("Auto step selector every_n_steps must be > 0");
      const double ratio = base_params.periodic_step_selector.phase_switch_ratio;
      if (!(ratio >= 0.0 && ratio <= 1.0)) throw std::invalid_argument("Auto step selector phase_switch_ratio must be within [0, 1]");
    }
    if ((initial || periodic) && base_params.learning_rate <= 0.0)
      throw std::invalid_argument("Step selectors require a positive base learning_rate");
    if (IsAlgorithm<LBFGSParams>() && spike_recovery_params.enable_rollback)
      throw std::invalid_argument("Spike rollback is not available with L-BFGS: the snapshot of the history ring is not built");
  }
  template <typename T> const T &GetAlgorithmParams() const { return std::get<T>(algorithm_params); }
  template <typename T> bool IsAlgorithm() const { return std::holds_alternative<T>(algorithm_params); }
  bool IsFirstOrder() const { return IsAlgorithm<SGDParams>() || IsAlgorithm<AdaGradParams>() || IsAlgorithm<AdamParams>(); }
};

// what an evaluator leaves behind for the optimizer: S_O / S_EO resident in the contractor's accumulators, the two sums on the host
template <typename TenElemT>
struct DeviceEvaluationT {
  TenElemT e_loc_sum = TenElemT(0.0);
  double weight_sum = 0.0;
  double energy_error = 0.0;
  std::vector<TenElemT> energy_samples;     // the local energy of every sample in the SR store, in its order (MinSR); empty: no sample set
  std::vector<double> accept_rates_avg;     // Monte-Carlo evaluators: mean acceptance rate of every walker over the evaluation's sweeps
  // what the evaluator's own anomaly checks found (AcceptanceRateCheck_, DetectEnergyErrorAnomaly_); empty: nothing
  std::vector<size_t> low_acceptance_walkers;      // walkers whose rate is below half the maximum over the walkers
  std::vector<size_t> nonfinite_sample_indices;    // the first (at most 5) samples of energy_samples that are not finite
};

template <typename TenElemT>
class Optimizer {
 public:
  using ContractorT = BMPSContractorT<TenElemT>;
  // evaluates the state the contractor holds; must not upload a state (TPSWaveFunctionComponentT::ResidentState)
  using Evaluator = std::function<DeviceEvaluationT<TenElemT>(ContractorT &)>;
  struct OptimizationCallback {
    std::function<void(size_t, double, double, double)> on_iteration;   // (iteration, energy, gradient norm, learning rate)
    // every evaluation that enters the trajectory, the closing one included, before the state moves: (the evaluation, its energy,
    // iteration).  Evaluations that spike recovery rejected and selector trials never get here.
    std::function<void(const DeviceEvaluationT<TenElemT> &, const TenElemT &, size_t)> on_evaluation_accepted;
    // after the step of an iteration: (iteration, energy, energy error) -> true ends the run without a closing evaluation (:888)
    std::function<bool(size_t, double, double)> should_stop;
  };
  struct OptimizationResult {
    std::vector<TenElemT> energy_trajectory;    // one entry per evaluation: max_iterations + 1 unless a criterion stopped the run
    std::vector<double> gradient_norms;
    TenElemT final_energy = TenElemT(0.0);
    double min_energy = std::numeric_limits<double>::max();
    size_t total_iterations = 0;                // update steps taken
    bool converged = false;
    size_t sr_iterations = 0;                   // of the last SR step
    double sr_natural_grad_norm = 0.0, sr_residual_norm = 0.0;
    // L-BFGS: the counters of the reference's optimizer, the evaluations its line searches made (they do not enter
    // energy_trajectory) and the step length of every iteration
    size_t lbfgs_skip_curvature_count = 0, lbfgs_damping_count = 0, lbfgs_descent_reset_count = 0, lbfgs_line_search_evaluations = 0;
    std::vector<double> learning_rate_trajectory;
    // spike recovery and step selectors.  The trajectories above hold accepted evaluations only.
    SpikeStatistics spike_stats;
    std::vector<double> energy_error_trajectory;    // one entry per entry of energy_trajectory
    std::vector<uint8_t> selector_triggered;        // per iteration: a step selector ran
    std::vector<double> selected_eta;               // per iteration: the learning rate it chose (0 where none ran)
    size_t evaluator_calls = 0, energy_only_calls = 0;   // calls of the evaluator (rejected ones, full-evaluator trials) / of the energy-only one
  };

  // adopts the state the contractor holds (UploadState first).  Fermionic states: the contractor holds the 4 d decorated components
  // and `fermion` carries the bond parities; the decoration is set on the context for the life of the optimizer.
  Optimizer(const OptimizerParams &params, ContractorT &contractor, const FermionDecoration *fermion = nullptr)
      : params_(params), c_(contractor), fermion_(fermion) {
    if (fermion_) {
      if (fermion_->bond_parity.empty()) throw std::invalid_argument("Optimizer: the FermionDecoration carries no bond parities");
      c_.FermionDecorationSet(fermion_->nf, fermion_->bond_parity);
    }
    try { c_.OptBegin(); } catch (...) { if (fermion_) pepsgpu_fermion_decoration_set(c_.ctx(), 0, nullptr, nullptr); throw; }
  }
  ~Optimizer() {
    pepsgpu_opt_end(c_.ctx());
    if (fermion_) pepsgpu_fermion_decoration_set(c_.ctx(), 0, nullptr, nullptr);
  }
  Optimizer(const Optimizer &) = delete;
  Optimizer &operator=(const Optimizer &) = delete;

  double GetCurrentLearningRate(size_t iteration, double current_energy) const {
    return params_.base_params.lr_scheduler ? params_.base_params.lr_scheduler->GetLearningRate(iteration, current_energy)
                                            : params_.base_params.learning_rate;
  }
  // the update rules on the device buffers: theta, the rule state and the device state move, the gradient buffer is read
  void SGDUpdate(double learning_rate, const SGDParams &p) { c_.OptStep(0, learning_rate, {p.momentum, p.nesterov ? 1.0 : 0.0, p.weight_decay}); }
  void AdaGradUpdate(double learning_rate) {
    const auto &p = params_.template GetAlgorithmParams<AdaGradParams>();
    c_.OptStep(1, learning_rate, {p.epsilon, p.initial_accumulator_value});
  }
  void AdamUpdate(double learning_rate, const AdamParams &p) { c_.OptStep(2, learning_rate, {p.beta1, p.beta2, p.epsilon, p.weight_decay}); }
  // natural gradient from the contractor's sample store (SRBegin / SRAppend), then theta -= lr x  (lr / |x| with normalize_update)
  typename ContractorT::NaturalGradientInfo StochasticReconfigurationUpdate(double learning_rate, const StochasticReconfigurationParams &p) {
    const auto &cg = p.cg_params;
    auto info = c_.OptNaturalGradient(p.diag_shift, cg.max_iter, cg.relative_tolerance, cg.absolute_tolerance, cg.residual_recompute_interval,
                                      cg.orthogonality_threshold);
    double step = learning_rate;
    if (p.normalize_update && info.direction_norm > 0.0) step /= info.direction_norm;
    c_.OptStep(0, step, {0.0, 0.0, 0.0});
    return info;
  }
  // MinSR direction from the contractor's sample store and the local energies of those samples (CalculateMinSRDirection_,
  // optimizer_impl.h:1126-1215), then theta -= lr x.  An evaluator that keeps no sample set (exact summation) leaves energy_samples empty.
  typename ContractorT::MinSRInfo MinSRUpdate(double learning_rate, const MinSRParams &p, const std::vector<TenElemT> &energy_samples,
                                              const TenElemT &energy) {
    if (energy_samples.size() != c_.SRCount() || energy_samples.empty())
      throw std::invalid_argument("Optimizer::MinSRUpdate: " + std::to_string(energy_samples.size()) + " local energies for " +
                                  std::to_string(c_.SRCount()) + " stored samples (MinSR needs an evaluator that keeps its sample set)");
    auto info = c_.MinSRDirection(energy_samples, energy, p.r_pinv, p.a_pinv, p.soft_cutoff);
    c_.OptStep(0, learning_rate, {0.0, 0.0, 0.0});
    return info;
  }
  // The two updates above in two halves, for spike recovery and the step selectors: the direction is left in the gradient buffer
  // (what S3 judges and the selector trials move along), and is applied later -- or never, when the evaluation is rejected.
  typename ContractorT::NaturalGradientInfo StochasticReconfigurationDirection(const StochasticReconfigurationParams &p) {
    const auto &cg = p.cg_params;
    return c_.OptNaturalGradient(p.diag_shift, cg.max_iter, cg.relative_tolerance, cg.absolute_tolerance, cg.residual_recompute_interval,
                                 cg.orthogonality_threshold);
  }
  typename ContractorT::MinSRInfo MinSRDirection(const MinSRParams &p, const std::vector<TenElemT> &energy_samples, const TenElemT &energy) {
    if (energy_samples.size() != c_.SRCount() || energy_samples.empty())
      throw std::invalid_argument("Optimizer::MinSRUpdate: " + std::to_string(energy_samples.size()) + " local energies for " +
                                  std::to_string(c_.SRCount()) + " stored samples (MinSR needs an evaluator that keeps its sample set)");
    return c_.MinSRDirection(energy_samples, energy, p.r_pinv, p.a_pinv, p.soft_cutoff);
  }
  // lr / |x| under normalize_update (SR only), once
  double AppliedDirectionStep(double learning_rate, double direction_norm) const {
    if (params_.template IsAlgorithm<StochasticReconfigurationParams>() &&
        params_.template GetAlgorithmParams<StochasticReconfigurationParams>().normalize_update && direction_norm > 0.0)
      return learning_rate / direction_norm;
    return learning_rate;
  }
  void ApplyDirection(double applied_step) { c_.OptStep(0, applied_step, {0.0, 0.0, 0.0}); }
  void ClipGradient() {                          // optimizer_impl.h:307-318
    if (!params_.IsFirstOrder()) return;
    const double cv = params_.base_params.clip_value.value_or(0.0), cn = params_.base_params.clip_norm.value_or(0.0);
    if (cv > 0.0 || cn > 0.0) c_.OptClip(cv, cn);
  }
  // `ev`, `energy`: the evaluation the gradient buffer was finished from (MinSR reads its local energies and their mean)
  void Update(double lr, OptimizationResult &res, const DeviceEvaluationT<TenElemT> &ev = DeviceEvaluationT<TenElemT>(),
              const TenElemT &energy = TenElemT(0.0)) {
    if (params_.template IsAlgorithm<SGDParams>()) SGDUpdate(lr, params_.template GetAlgorithmParams<SGDParams>());
    else if (params_.template IsAlgorithm<AdaGradParams>()) AdaGradUpdate(lr);
    else if (params_.template IsAlgorithm<AdamParams>()) AdamUpdate(lr, params_.template GetAlgorithmParams<AdamParams>());
    else if (params_.template IsAlgorithm<StochasticReconfigurationParams>()) {
      auto info = StochasticReconfigurationUpdate(lr, params_.template GetAlgorithmParams<StochasticReconfigurationParams>());
      res.sr_iterations = (size_t)info.iterations; res.sr_natural_grad_norm = info.direction_norm; res.sr_residual_norm = info.residual_norm;
    } else if (params_.template IsAlgorithm<MinSRParams>()) {
      // sr_iterations and sr_residual_norm stay 0: there is no iterative solve (the reference's IterationRecord says the same)
      last_minsr_ = MinSRUpdate(lr, params_.template GetAlgorithmParams<MinSRParams>(), ev.energy_samples, energy);
      res.sr_natural_grad_norm = last_minsr_.direction_norm;
    } else {
      throw std::logic_error("Optimizer::Update: no update rule for this alternative of AlgorithmParams");
    }
  }
  const typename ContractorT::MinSRInfo &LastMinSRInfo() const { return last_minsr_; }
  bool ShouldStop(double current_energy, double previous_energy, double gradient_norm, size_t iterations_without_improvement) const {   // :1764-1793
    const auto &b = params_.base_params;
    return gradient_norm < b.gradient_tolerance || std::abs(current_energy - previous_energy) < b.energy_tolerance ||
           iterations_without_improvement >= b.plateau_patience;
  }
  // StrongWolfeLBFGSStep_ (optimizer_impl.h:1547-1662) on the direction and base the device holds: every trial is one element-wise
  // pass (theta = theta_base + alpha d), `evaluate_trial` (phi, the gradient buffer) and one dot product (phi').  Returns the
  // accepted step length with theta at that point, or a negative value with theta wherever the last trial left it.
  double StrongWolfeLBFGSStep(const std::function<double()> &evaluate_trial, double learning_rate, const LBFGSParams &p, double phi0,
                              double dphi0, size_t &eval_count) {
    if (p.wolfe_c1 <= 0.0 || p.wolfe_c1 >= 1.0 || p.wolfe_c2 <= p.wolfe_c1 || p.wolfe_c2 >= 1.0)
      throw std::invalid_argument("LBFGS strong-Wolfe parameters must satisfy 0 < c1 < c2 < 1");
    if (p.max_eval == 0) throw std::invalid_argument("LBFGS max_eval must be > 0 for strong-Wolfe mode");
    if (p.tolerance_grad < 0.0) throw std::invalid_argument("LBFGS tolerance_grad must be >= 0 for strong-Wolfe mode");
    if (dphi0 >= 0.0) return -1.0;
    const double curvature_threshold = std::max(-p.wolfe_c2 * dphi0, p.tolerance_grad);
    eval_count = 0;
    auto eval_alpha = [&](double alpha, double *phi, double *dphi) {
      c_.LBFGSTrial(alpha);
      *phi = evaluate_trial();
      *dphi = c_.LBFGSSlope();
      ++eval_count;
    };
    auto zoom = [&](double alo, double phi_alo, double ahi) -> double {
      while (eval_count < p.max_eval) {
        const double alpha = 0.5 * (alo + ahi);
        double phi = 0.0, dphi = 0.0;
        eval_alpha(alpha, &phi, &dphi);
        if ((phi > phi0 + p.wolfe_c1 * alpha * dphi0) || (phi >= phi_alo)) {
          ahi = alpha;
        } else {
          if (std::abs(dphi) <= curvature_threshold) return alpha;
          if (dphi * (ahi - alo) >= 0.0) ahi = alo;
          alo = alpha;
          phi_alo = phi;
        }
        if (std::abs(ahi - alo) <= p.tolerance_change) break;
      }
      return -1.0;
    };
    double alpha_prev = 0.0, phi_prev = phi0;
    double alpha = std::clamp(std::max(learning_rate, p.min_step), p.min_step, p.max_step);
    if (alpha <= 0.0) alpha = p.min_step;
    for (size_t outer = 0; eval_count < p.max_eval; ++outer) {
      double phi = 0.0, dphi = 0.0;
      eval_alpha(alpha, &phi, &dphi);
      if ((phi > phi0 + p.wolfe_c1 * alpha * dphi0) || (outer > 0 && phi >= phi_prev)) return zoom(alpha_prev, phi_prev, alpha);
      if (std::abs(dphi) <= curvature_threshold) return alpha;
      if (dphi >= 0.0) return zoom(alpha, phi, alpha_prev);
      alpha_prev = alpha;
      phi_prev = phi;
      const double next_alpha = std::min(alpha * 2.0, p.max_step);
      if (next_alpha - alpha <= p.tolerance_change) break;
      alpha = next_alpha;
    }
    return -1.0;
  }
  // The L-BFGS schedule of IterativeOptimize (optimizer_impl.h:244-249, 619-675, 847-857): evaluate -> history update from the anchor
  // -> direction (with the descent reset) -> fixed step or strong-Wolfe search -> the anchor becomes the point the step left.  The
  // accepted point is evaluated again by the next iteration, as in the reference; the gradient is not clipped (:311 is first-order
  // only).  A failed search restores theta and throws std::runtime_error unless allow_fallback_to_fixed_step is set.
  OptimizationResult IterativeOptimizeLBFGS_(const Evaluator &evaluator, const OptimizationCallback &callback) {
    const LBFGSParams &p = params_.template GetAlgorithmParams<LBFGSParams>();
    if (p.history_size == 0) throw std::invalid_argument("LBFGS history_size must be > 0");
    c_.LBFGSBegin(p.history_size);
    OptimizationResult res;
    double previous_energy = 0.0;
    size_t without_improvement = 0;
    auto counters = [&]() {
      const auto k = c_.LBFGSGetCounters();
      res.lbfgs_skip_curvature_count = k.skip_curvature; res.lbfgs_damping_count = k.damping; res.lbfgs_descent_reset_count = k.descent_reset;
    };
    // Spike recovery (deviation from the reference, which judges after its history update and restores the ring): S1 / S2 are judged
    // before LBFGSUpdate, so a rejected evaluation never reaches the ring and evaluating again needs no restore.  The trials of the
    // line search bypass detection, as in the reference.  Rollback is refused (OptimizerParams::ValidateGuards).
    SpikeGuard guard(params_.spike_recovery_params);
    DeviceEvaluationT<TenElemT> ev;
    auto evaluate = [&]() {
      ev = evaluator(c_);
      ++res.evaluator_calls;
      return c_.OptGradientFromAccumulators(ev.e_loc_sum, ev.weight_sum);
    };
    auto record = [&](const std::pair<TenElemT, double> &eg, size_t iter) {
      res.energy_trajectory.push_back(eg.first);
      res.gradient_norms.push_back(eg.second);
      res.energy_error_trajectory.push_back(ev.energy_error);
      res.final_energy = eg.first;
      if (callback.on_evaluation_accepted) callback.on_evaluation_accepted(ev, eg.first, iter);
    };
    auto finish = [&]() {
      counters();
      res.spike_stats = guard.Statistics();
      guard.WriteTriggerCsvFile();
    };
    for (size_t iter = 0; iter < params_.base_params.max_iterations; ++iter) {
      auto eg = evaluate();
      for (size_t attempts = 0; guard.JudgeEvaluation(iter, attempts, ev.energy_error, eg.second) == SpikeAction::kResample; ++attempts)
        eg = evaluate();
      guard.Accept(std::real(eg.first), ev.energy_error, eg.second, nullptr);
      record(eg, iter);
      const double e = std::real(eg.first);
      if (e < res.min_energy) { res.min_energy = e; without_improvement = 0; } else ++without_improvement;
      const double lr = GetCurrentLearningRate(iter, iter == 0 ? e : previous_energy);
      if (callback.on_iteration) callback.on_iteration(iter, e, eg.second, lr);
      c_.LBFGSUpdate(p.min_curvature, p.use_damping);
      if (iter > 0 && ShouldStop(e, previous_energy, eg.second, without_improvement)) { res.converged = true; finish(); return res; }
      const double accepted_error = ev.energy_error;      // (the line search evaluates through `ev`)
      const auto dir = c_.LBFGSDirection(p.min_curvature, p.max_direction_norm);
      double used_step = 0.0;
      if (p.step_mode == LBFGSStepMode::kFixed) {
        used_step = std::max(0.0, lr);                                  // ApplyFixedLBFGSStep_, :1534-1545
        c_.LBFGSTrial(used_step);
      } else {
        size_t evals = 0;
        double alpha = -1.0;
        try {
          alpha = StrongWolfeLBFGSStep([&]() { return std::real(evaluate().first); }, lr, p, e, dir.dphi0, evals);
        } catch (...) {
          res.lbfgs_line_search_evaluations += evals;
          if (evals > 0) c_.LBFGSTrial(0.0);
          throw;
        }
        res.lbfgs_line_search_evaluations += evals;
        if (alpha >= 0.0) {
          used_step = alpha;
        } else if (p.allow_fallback_to_fixed_step) {
          used_step = std::max(0.0, std::max(p.min_step, lr * p.fallback_fixed_step_scale));
          c_.LBFGSTrial(used_step);
        } else {
          c_.LBFGSTrial(0.0);                                           // theta_base bit for bit
          throw std::runtime_error("L-BFGS strong-Wolfe line search failed. "
                                   "Set allow_fallback_to_fixed_step=true for explicit fixed-step fallback.");
        }
      }
      c_.LBFGSCommit();
      res.learning_rate_trajectory.push_back(used_step);
      if (params_.base_params.lr_scheduler) params_.base_params.lr_scheduler->Step();
      previous_energy = e;
      res.total_iterations = iter + 1;
      if (callback.should_stop && callback.should_stop(iter, e, accepted_error)) { finish(); return res; }
      SaveCheckpoint_(iter, res.energy_trajectory, res.energy_error_trajectory);
    }
    const auto eg = evaluate();
    record(eg, params_.base_params.max_iterations);
    res.min_energy = std::min(res.min_energy, std::real(eg.first));
    finish();
    return res;
  }
  // evaluate -> finish -> clip -> [natural gradient] -> step, max_iterations times, then one closing evaluation.  Around that, all
  // off by default: spike recovery (S1-S4 with resampling and rollback), the step selectors and checkpoints, in the order of
  // optimizer_impl.h:233-900.  With the three off the device calls are exactly the line above.
  //   1. evaluate, finish (energy, |g|)                    2. S1 / S2: evaluate again, or restore the base and evaluate again
  //   3. learning rate                                     4. SR / MinSR: the direction only
  //   5. S3 on |x| and the CG iterations                   6. S4: always a rollback
  //   7. clip; step selector: trials theta_base - eta d, each restored
  //   8. accept: trackers, trajectories, lowest energy, stopping, callbacks, base <- theta, THEN the rule kernel / the direction
  //      applied, checkpoint
  // Deviations from the reference, each on purpose:
  //   - The rule kernel runs after the S4 decision (the reference computes updated_state before S3 / S4 and so advances the Adam /
  //     AdaGrad / momentum state for a step it then throws away; it lists that as a known limitation).  Here no rejected evaluation
  //     touches rule state, and an S3 resample cannot update it twice.
  //   - A selector trial never moves theta for good: OptPreview forms the trial from the saved base on the device and OptBaseRestore
  //     puts the base back bit for bit; the real step then starts from it.  A trial with the full evaluator overwrites the
  //     accumulators but not the gradient buffer, so the direction (precomputed_natural_direction) is still there to apply.
  //   - S3 and S4 are judged before the selector's trials, not after them.  Neither verdict reads anything the trials produce, so the
  //     accepted trajectory is the same; a rejected evaluation costs no trials and does not move the selector's base learning rate,
  //     and the one base buffer in HBM is free for the trials exactly when no rollback can follow in the same pass.
  //   - The closing evaluation after the last step bypasses detection and the trackers; it is recorded as before.
  // `energy_only_evaluator` (optional) serves the selector trials; it leaves only e_loc_sum, weight_sum and energy_error.
  OptimizationResult IterativeOptimize(const Evaluator &evaluator, const OptimizationCallback &callback = OptimizationCallback(),
                                       const Evaluator &energy_only_evaluator = Evaluator()) {
    params_.ValidateGuards();                      // before any device call
    if (params_.template IsAlgorithm<LBFGSParams>()) return IterativeOptimizeLBFGS_(evaluator, callback);
    const auto &b = params_.base_params;
    const auto &spike = params_.spike_recovery_params;
    const bool is_sgd = params_.template IsAlgorithm<SGDParams>(), is_sr = params_.template IsAlgorithm<StochasticReconfigurationParams>(),
               is_minsr = params_.template IsAlgorithm<MinSRParams>();
    const bool any_selector = b.initial_step_selector.enabled || b.periodic_step_selector.enabled;
    double selector_base_lr = b.learning_rate;
    SpikeGuard guard(spike);
    OptimizationResult res;
    double previous_energy = 0.0;
    size_t without_improvement = 0;
    DeviceEvaluationT<TenElemT> ev;
    auto evaluate = [&]() {
      ev = evaluator(c_);
      ++res.evaluator_calls;
      return c_.OptGradientFromAccumulators(ev.e_loc_sum, ev.weight_sum);
    };
    auto record = [&](const std::pair<TenElemT, double> &eg, size_t iter) {
      res.energy_trajectory.push_back(eg.first);
      res.gradient_norms.push_back(eg.second);
      res.energy_error_trajectory.push_back(ev.energy_error);
      res.final_energy = eg.first;
      if (callback.on_evaluation_accepted) callback.on_evaluation_accepted(ev, eg.first, iter);
    };
    auto finish = [&]() {
      res.spike_stats = guard.Statistics();
      guard.WriteTriggerCsvFile();
    };
    // one trial of a selector: the energy (and error) of the state the device holds
    auto trial_energy = [&]() {
      DeviceEvaluationT<TenElemT> t;
      if (energy_only_evaluator) { t = energy_only_evaluator(c_); ++res.energy_only_calls; }
      else { t = evaluator(c_); ++res.evaluator_calls; }       // (its gradient stays in the accumulators, unfinished)
      return std::make_pair(std::real(t.e_loc_sum / t.weight_sum), t.energy_error);
    };
    for (size_t iter = 0; iter < b.max_iterations; ++iter) {
      size_t attempts = 0;
      for (;;) {
        const auto eg = evaluate();
        const double e = std::real(eg.first);
        // rollback: theta <- the last accepted state, which is then evaluated again; with no base saved just evaluate again
        auto rollback = [&]() {
          if (guard.TakeBase()) { c_.OptBaseRestore(); c_.OptBaseClear(); }
          attempts = 0;
        };
        SpikeAction action = guard.JudgeEvaluation(iter, attempts, ev.energy_error, eg.second);
        if (action == SpikeAction::kResample) { ++attempts; continue; }
        if (action == SpikeAction::kRollback) { rollback(); continue; }
        double lr = any_selector ? selector_base_lr : GetCurrentLearningRate(iter, iter == 0 ? e : previous_energy);
        bool clipped = false, have_direction = false;
        auto clip_once = [&]() { if (!clipped) { ClipGradient(); clipped = true; } };
        typename ContractorT::NaturalGradientInfo sr_info;
        double direction_norm = 0.0;
        auto direction_once = [&]() {
          if (have_direction) return;
          if (is_sr) {
            sr_info = StochasticReconfigurationDirection(params_.template GetAlgorithmParams<StochasticReconfigurationParams>());
            direction_norm = sr_info.direction_norm;
          } else {
            last_minsr_ = MinSRDirection(params_.template GetAlgorithmParams<MinSRParams>(), ev.energy_samples, eg.first);
            direction_norm = last_minsr_.direction_norm;
          }
          have_direction = true;
        };
        if ((is_sr || is_minsr) && spike.enable_auto_recover) {
          direction_once();
          action = guard.JudgeDirection(iter, attempts, direction_norm, is_minsr ? std::numeric_limits<size_t>::max() : (size_t)sr_info.iterations);
          if (action == SpikeAction::kResample) { ++attempts; continue; }
          if (action == SpikeAction::kRollback) { rollback(); continue; }
        }
        if (guard.JudgeEnergy(iter, attempts, e) == SpikeAction::kRollback) { rollback(); continue; }
        const bool initial_triggered = b.initial_step_selector.enabled && iter == 0;
        const bool periodic_triggered = b.periodic_step_selector.enabled && iter > 0 && iter % b.periodic_step_selector.every_n_steps == 0;
        const bool selector_triggered = initial_triggered || periodic_triggered;
        if (selector_triggered) {
          const bool need_error = initial_triggered ? !b.initial_step_selector.enable_in_deterministic
                                                    : !b.periodic_step_selector.enable_in_deterministic;
          if (need_error && ev.energy_error <= 0.0)
            throw std::invalid_argument(std::string(initial_triggered ? "Initial" : "Auto") +
                                        " step selector requires positive energy error in MC mode. "
                                        "Set enable_in_deterministic=true to allow deterministic evaluators.");
          const std::vector<double> etas = StepCandidates(initial_triggered, selector_base_lr, b.initial_step_selector.max_line_search_steps);
          std::vector<double> sgd;
          if (is_sgd) {
            const auto &p = params_.template GetAlgorithmParams<SGDParams>();
            sgd = {p.momentum, p.nesterov ? 1.0 : 0.0, p.weight_decay};
            clip_once();
          } else {
            sgd = {0.0, 0.0, 0.0};
            direction_once();
          }
          c_.OptBaseSave();
          std::vector<StepCandidateResult> results;
          try {
            for (const double eta : etas) {
              c_.OptPreview(is_sgd ? eta : AppliedDirectionStep(eta, direction_norm), sgd);
              const auto t = trial_energy();
              CheckStepCandidate(t.first, t.second);
              results.push_back({eta, t.first, t.second});
            }
          } catch (...) {
            c_.OptBaseRestore();
            if (!guard.HasBase()) c_.OptBaseClear();
            throw;
          }
          c_.OptBaseRestore();
          if (!guard.HasBase()) c_.OptBaseClear();      // (the trials' base is no rollback target)
          const double selected = initial_triggered ? SelectInitialStep(results)
                                                    : SelectPeriodicStep(results, iter, b.max_iterations, b.periodic_step_selector.phase_switch_ratio);
          if (initial_triggered && selected != selector_base_lr)
            std::cout << "[INITIAL_STEP] Iter 0: selected step size " << selector_base_lr << " -> " << selected << std::endl;
          if (periodic_triggered && selected < selector_base_lr)
            std::cout << "[PERIODIC_STEP] Iter " << iter << ": step size halved " << selector_base_lr << " -> " << selected << std::endl;
          selector_base_lr = NextSelectorBaseLR(initial_triggered, selector_base_lr, selected);
          lr = selector_base_lr;
        }
        // ---- accepted ----
        guard.Accept(e, ev.energy_error, eg.second, have_direction ? &direction_norm : nullptr);
        record(eg, iter);
        if (e < res.min_energy) { res.min_energy = e; without_improvement = 0; } else ++without_improvement;
        if (callback.on_iteration) callback.on_iteration(iter, e, eg.second, lr);
        if (iter > 0 && ShouldStop(e, previous_energy, eg.second, without_improvement)) { res.converged = true; finish(); return res; }
        if (spike.enable_rollback) { c_.OptBaseSave(); guard.MarkBaseSaved(); }
        clip_once();
        if (have_direction) {
          ApplyDirection(AppliedDirectionStep(lr, direction_norm));
          res.sr_natural_grad_norm = direction_norm;
          if (is_sr) { res.sr_iterations = (size_t)sr_info.iterations; res.sr_residual_norm = sr_info.residual_norm; }
        } else {
          Update(lr, res, ev, eg.first);
        }
        res.selector_triggered.push_back(selector_triggered ? 1 : 0);
        res.selected_eta.push_back(selector_triggered ? lr : 0.0);
        if (b.lr_scheduler) params_.base_params.lr_scheduler->Step();
        previous_energy = e;
        res.total_iterations = iter + 1;
        if (callback.should_stop && callback.should_stop(iter, e, ev.energy_error)) { finish(); return res; }
        SaveCheckpoint_(iter, res.energy_trajectory, res.energy_error_trajectory);
        break;
      }
    }
    const auto eg = evaluate();
    record(eg, b.max_iterations);
    res.min_energy = std::min(res.min_energy, std::real(eg.first));
    finish();
    return res;
  }
  // SaveCheckpoint_ / WriteTrajectoryCsv_ (optimizer_impl.h:1980-2049): base_path/step_{k}/ holds the state after step k (read from
  // theta; fermionic states: the stored tensors), checkpoint_meta.txt and trajectory_snapshot.csv; base_path/energy_trajectory.csv is
  // rewritten every time.  The extents are the contractor's.
  void SaveCheckpoint_(size_t step, const std::vector<TenElemT> &energy_traj, const std::vector<double> &error_traj) const {
    const auto &cfg = params_.checkpoint_params;
    if (!cfg.IsEnabled() || step == 0 || step % cfg.every_n_steps != 0) return;
    const std::string dir = cfg.base_path + "/step_" + std::to_string(step);
    EnsureDirectoryExists(dir);
    GetState(c_.rows(), c_.cols(), fermion_ ? c_.phys_dim() / 4 : c_.phys_dim(), c_.bond_dim()).Dump(dir);
    {
      std::ofstream meta(dir + "/checkpoint_meta.txt");
      if (!meta) throw std::ios_base::failure("Optimizer: failed to open " + dir + "/checkpoint_meta.txt");
      meta << "step " << step << "\n";
      if (!energy_traj.empty()) meta << "energy " << std::setprecision(17) << std::real(energy_traj.back()) << "\n";
      if (!error_traj.empty()) meta << "error " << std::setprecision(17) << error_traj.back() << "\n";
    }
    WriteTrajectoryCsv_(dir + "/trajectory_snapshot.csv", energy_traj, error_traj);
    WriteTrajectoryCsv_(cfg.base_path + "/energy_trajectory.csv", energy_traj, error_traj);
    std::cout << "[CHECKPOINT] Saved step " << step << " to " << dir << std::endl;
  }
  static void WriteTrajectoryCsv_(const std::string &path, const std::vector<TenElemT> &energy_traj, const std::vector<double> &error_traj) {
    std::ofstream csv(path);
    if (!csv) throw std::runtime_error("Failed to write trajectory CSV file '" + path + "'");
    csv << "iteration,energy,energy_error\n";
    for (size_t i = 0; i < energy_traj.size(); ++i)
      csv << i << "," << std::setprecision(17) << std::real(energy_traj[i]) << "," << (i < error_traj.size() ? error_traj[i] : 0.0) << "\n";
    if (!csv) throw std::runtime_error("Failed to write trajectory CSV file '" + path + "'");
  }
  // phys_dim: the components of the caller's state -- for a fermionic state the d stored ones (variant 0 of the device's 4 d)
  SplitIndexTPST<TenElemT> GetState(size_t rows, size_t cols, size_t phys_dim, size_t D) const {
    if (!fermion_) {
      SplitIndexTPST<TenElemT> s(rows, cols, phys_dim, D);
      c_.OptReadState(s);
      return s;
    }
    SplitIndexTPST<TenElemT> ext(rows, cols, 4 * phys_dim, D), s(rows, cols, phys_dim, D);
    c_.OptReadState(ext);
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < cols; ++c)
        for (size_t k = 0; k < phys_dim; ++k) std::copy(ext.component(r, c, k), ext.component(r, c, k) + ext.slot(), s.component(r, c, k));
    return s;
  }

 private:
  OptimizerParams params_;
  ContractorT &c_;
  const FermionDecoration *fermion_ = nullptr;
  typename ContractorT::MinSRInfo last_minsr_;
};

// what AccumulateDevice of the gradient accumulator hands the device for one batch: bosons the amplitudes, fermions the dense
// (undecorated-sign) amplitudes sigma * psi and the extended row-major states the holes belong to
template <typename TenElemT>
void ResidentGradAccumulate(TPSWaveFunctionComponentT<TenElemT> &comp, const EnergyAndHolesT<TenElemT> &eh, bool exact_sum, bool sr_append) {
  if (!comp.fermion) {
    comp.contractor.GradAccumulate(comp.amplitude, eh.energy, exact_sum);
    if (sr_append) comp.contractor.SRAppend(comp.amplitude);
    return;
  }
  std::vector<TenElemT> dense(comp.amplitude);
  for (size_t w = 0; w < dense.size(); ++w) dense[w] *= double(comp.fermion->Sigma(comp.config, w));
  const Configuration ext = comp.fermion->ExtConfig(comp.config, ROW_MAJOR);
  comp.contractor.GradAccumulate(dense, eh.energy, exact_sum, std::vector<int32_t>(ext.data(), ext.data() + ext.walkers() * ext.rows() * ext.cols()));
  if (sr_append) {        // the sample store takes the components from the walkers' table: the column pass left the column-major one
    comp.contractor.Init(ext);
    comp.contractor.SRAppend(dense);
  }
}

// The accumulation of ExactSumEnergyEvaluator for the state the device holds: S_O / S_EO stay in HBM, the two sums come back.
// `shape` gives the extents only.  One rank.
template <typename ModelT, typename TenElemT>
DeviceEvaluationT<TenElemT> ExactSumAccumulateResident(const SplitIndexTPST<TenElemT> &shape, const std::vector<std::vector<int32_t>> &all_configs,
                                                      BMPSContractorT<TenElemT> &contractor, ModelT &model, size_t batch,
                                                      const FermionDecoration *fermion = nullptr) {
  const size_t rows = shape.rows(), cols = shape.cols();
  DeviceEvaluationT<TenElemT> ev;
  contractor.GradReset();
  for (size_t b0 = 0; b0 < all_configs.size(); b0 += batch) {
    const size_t nb = std::min(batch, all_configs.size() - b0);
    Configuration cfg(nb, rows, cols);
    for (size_t w = 0; w < nb; ++w) std::copy(all_configs[b0 + w].begin(), all_configs[b0 + w].end(), cfg.data() + w * rows * cols);
    TPSWaveFunctionComponentT<TenElemT> comp(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), cfg, contractor, fermion);
    EnergyAndHolesT<TenElemT> eh = model.template CalEnergyAndHoles<true>(shape, comp, /*holes_on_device=*/true);
    ResidentGradAccumulate(comp, eh, true, false);
    for (size_t w = 0; w < nb; ++w) {
      const double wt = AbsSquare(comp.amplitude[w]);
      ev.weight_sum += wt;
      ev.e_loc_sum += eh.energy[w] * wt;
    }
  }
  return ev;
}

// The accumulation of MCEnergyGradEvaluator (mc_energy_grad_evaluator.h:245-278) over a given set of samples with weight 1, for the
// state the device holds: S_O / S_EO in the accumulators and the O* samples in the SR store (what the SR step solves with), both in HBM.
template <typename ModelT, typename TenElemT>
DeviceEvaluationT<TenElemT> SampleSetAccumulateResident(const SplitIndexTPST<TenElemT> &shape, const Configuration &samples,
                                                       BMPSContractorT<TenElemT> &contractor, ModelT &model,
                                                       const FermionDecoration *fermion = nullptr) {
  DeviceEvaluationT<TenElemT> ev;
  contractor.GradReset();
  contractor.SRBegin(samples.walkers());
  TPSWaveFunctionComponentT<TenElemT> comp(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), samples, contractor, fermion);
  EnergyAndHolesT<TenElemT> eh = model.template CalEnergyAndHoles<true>(shape, comp, /*holes_on_device=*/true);
  ResidentGradAccumulate(comp, eh, false, true);
  for (size_t w = 0; w < samples.walkers(); ++w) { ev.weight_sum += 1.0; ev.e_loc_sum += eh.energy[w]; }
  ev.energy_samples = eh.energy;
  return ev;
}

// ---------------------------------------------------------------------------------------------
// Monte-Carlo VMC on the resident state: the evaluator of the reference's example programs and the executor around the Optimizer.

// MeanAndBinnedErrorSqrtNUniformBin (vmc_basic/monte_carlo_tools/statistics.h:146-225) with a walker in the role of an MPI rank.
// samples: [sample][walker] (sample-major, walker-minor: the order MCEnergyGradEvaluator fills energy_samples).  Per walker the bin
// size is max(1, floor(sqrt(S))), trailing samples that fill no bin are dropped (:159-162); the bin means are gathered walker-major
// (:203-207); their mean is the energy and their standard error the error, one bin in total gives an infinite error (:213-222).
template <typename TenElemT>
inline std::pair<TenElemT, double> MeanAndBinnedErrorSqrtNUniformBin(const std::vector<TenElemT> &samples, size_t n_walkers) {
  if (n_walkers == 0 || samples.size() % n_walkers != 0)
    throw std::invalid_argument("MeanAndBinnedErrorSqrtNUniformBin: samples must be [sample][walker] with at least one walker");
  const size_t S = samples.size() / n_walkers;
  std::vector<TenElemT> bins;
  if (S > 0) {
    const size_t bin_size = std::max<size_t>(1, static_cast<size_t>(std::sqrt((double)S)));
    const size_t num_bins = S / bin_size;
    bins.reserve(num_bins * n_walkers);
    for (size_t w = 0; w < n_walkers; ++w)
      for (size_t i = 0; i < num_bins; ++i) {
        TenElemT bin_sum(0.0);
        for (size_t k = i * bin_size; k < (i + 1) * bin_size; ++k) bin_sum += samples[k * n_walkers + w];
        bins.push_back(bin_sum / double(bin_size));
      }
  }
  TenElemT mean(0.0);
  double err = 0.0;
  if (!bins.empty()) {
    for (const auto &b : bins) mean += b;                        // Mean (:51-59)
    mean /= double(bins.size());
    if (bins.size() > 1) {
      double sq = 0.0;
      for (const auto &b : bins) sq += std::norm(b - mean);      // Variance (:61-81), StandardError (:88-96)
      err = std::sqrt(sq / double(bins.size()) / (double(bins.size()) - 1.0));
    } else {
      err = std::numeric_limits<double>::infinity();
    }
  }
  return {mean, err};
}

// AcceptanceRateCheck_ (mc_energy_grad_evaluator.h:401-420) with a walker in the role of an MPI rank: the walkers whose mean
// acceptance rate is below half the maximum over the walkers
inline std::vector<size_t> AcceptanceRateCheck(const std::vector<double> &rates) {
  std::vector<size_t> flagged;
  if (rates.empty()) return flagged;
  const double mx = *std::max_element(rates.begin(), rates.end());
  for (size_t w = 0; w < rates.size(); ++w)
    if (rates[w] < 0.5 * mx) flagged.push_back(w);
  return flagged;
}
// DetectEnergyErrorAnomaly_ (:437-470): an infinite error although the binning had more than one bin to work with; returns the
// indices of the first (at most 5) non-finite samples
template <typename TenElemT>
inline std::vector<size_t> DetectEnergyErrorAnomaly(double energy_error, size_t samples_per_walker, size_t n_walkers,
                                                    const std::vector<TenElemT> &energy_samples, bool *anomalous = nullptr) {
  std::vector<size_t> bad;
  if (anomalous) *anomalous = false;
  if (!std::isinf(energy_error)) return bad;
  const size_t bin_size = std::max<size_t>(1, static_cast<size_t>(std::sqrt((double)samples_per_walker)));
  if (n_walkers * (samples_per_walker / bin_size) <= 1) return bad;
  if (anomalous) *anomalous = true;
  for (size_t i = 0; i < energy_samples.size() && bad.size() < 5; ++i)
    if (!std::isfinite(std::real(energy_samples[i])) || !std::isfinite(std::imag(energy_samples[i]))) bad.push_back(i);
  return bad;
}

// MCEnergyGradEvaluator (algorithm/vmc_update/mc_energy_grad_evaluator.h:152-330) for the state the device holds.  It owns nothing
// but references: the engine (resident mode), the model, the decoration of a fermionic state and the Monte-Carlo parameters.
// Evaluate(contractor) is an Optimizer::Evaluator: S_O / S_EO stay in the contractor's accumulators, the O* samples in its SR store
// (collect_sr_buffers: SR, MinSR), the energies come back.  The chains persist from one Evaluate to the next: configurations and the
// updater's engines are never re-seeded; only the environments are rebuilt on the stepped state (RefreshWavefunctionComponent, :164).
// One rank; a walker plays the role of an MPI rank in the statistics and in the acceptance-rate anomaly check (:289, :382), whose
// findings and those of the energy-error anomaly check (:319) come back in the evaluation and go to std::cerr, at most
// kMaxAnomalyReports times per evaluator.  EvaluateEnergyOnly (:343-392) serves the step selectors' trials: sweeps and local energies
// only, no accumulators, no sample store.  Not built: the psi-consistency warning policy (:219-244).
template <class MonteCarloSweepUpdater, class Model, typename TenElemT = double>
class MCEnergyGradEvaluator {
 public:
  using ContractorT = BMPSContractorT<TenElemT>;
  using EngineT = MonteCarloEngine<MonteCarloSweepUpdater, TenElemT>;
  MCEnergyGradEvaluator(EngineT &engine, Model &model, const MonteCarloParams &params, bool collect_sr_buffers,
                        const FermionDecoration *fermion = nullptr)
      : engine_(engine), model_(model), fermion_(fermion), params_(params), collect_sr_buffers_(collect_sr_buffers) {
    if (params_.samples_per_walker == 0) throw std::invalid_argument("MCEnergyGradEvaluator: samples_per_walker must be positive");
    if (engine_.WavefuncComp().fermion != fermion_)
      throw std::invalid_argument("MCEnergyGradEvaluator: the decoration is not the one of the engine's wave-function component");
    if (IsFermionicModel<Model>::value != (fermion_ != nullptr))
      throw std::invalid_argument("MCEnergyGradEvaluator: a fermionic model needs a FermionDecoration, a bosonic one takes none");
  }
  DeviceEvaluationT<TenElemT> Evaluate(ContractorT &contractor) {
    auto &comp = engine_.WavefuncComp();
    if (&contractor != &comp.contractor) throw std::invalid_argument("MCEnergyGradEvaluator: not the contractor of the engine's walkers");
    const size_t n = comp.config.walkers(), S = params_.samples_per_walker;
    engine_.RefreshWavefunctionComponent();        // :164 -- do NOT normalise here: that would rescale the gradient
    contractor.GradReset();
    if (collect_sr_buffers_) contractor.SRBegin(n * S);
    DeviceEvaluationT<TenElemT> ev;
    ev.energy_samples.reserve(n * S);
    ev.accept_rates_avg.assign(n, 0.0);
    for (size_t k = 0; k < S; ++k) {               // :205-282
      const std::vector<double> rates = engine_.StepSweep();
      for (size_t w = 0; w < n && w < rates.size(); ++w) ev.accept_rates_avg[w] += rates[w];
      EnergyAndHolesT<TenElemT> eh = model_.template CalEnergyAndHoles<true>(engine_.State(), comp, /*holes_on_device=*/true);
      ResidentGradAccumulate(comp, eh, false, collect_sr_buffers_);
      ev.energy_samples.insert(ev.energy_samples.end(), eh.energy.begin(), eh.energy.end());   // sample-major, walker-minor: the store's order
    }
    for (auto &r : ev.accept_rates_avg) r /= double(S);                                       // :285-286
    const auto stat = MeanAndBinnedErrorSqrtNUniformBin(ev.energy_samples, n);                 // :292
    ev.weight_sum = double(n * S);
    // As in the reference (:292-298) the gradient is formed with the BINNED energy, which drops the trailing samples of every walker,
    // while the O* sums run over all samples: grad = S_EO / W - conj(E_binned) S_O / W.  The optimizer finishes the gradient with
    // E = e_loc_sum / weight_sum, so hand it E_binned * W instead of the plain sum of the local energies.
    ev.e_loc_sum = stat.first * ev.weight_sum;
    ev.energy_error = stat.second;
    ReportLowAcceptance_(ev);                                                                  // :289
    bool anomalous = false;                                                                    // :319
    ev.nonfinite_sample_indices = DetectEnergyErrorAnomaly(ev.energy_error, S, n, ev.energy_samples, &anomalous);
    if (anomalous && reports_++ < kMaxAnomalyReports) {
      std::cerr << "Energy error is infinite with " << n << " walkers x " << S << " samples: NaNs or identical samples.";
      for (const size_t i : ev.nonfinite_sample_indices) std::cerr << " non-finite energy_samples[" << i << "] = " << ev.energy_samples[i] << ";";
      std::cerr << std::endl;
    }
    return ev;
  }
  // the energy and its error of the state the device holds, for a step-selector trial: the chains go on from where they are
  DeviceEvaluationT<TenElemT> EvaluateEnergyOnly(ContractorT &contractor) {
    auto &comp = engine_.WavefuncComp();
    if (&contractor != &comp.contractor) throw std::invalid_argument("MCEnergyGradEvaluator: not the contractor of the engine's walkers");
    const size_t n = comp.config.walkers(), S = params_.samples_per_walker;
    engine_.RefreshWavefunctionComponent();
    DeviceEvaluationT<TenElemT> ev;
    std::vector<TenElemT> samples;
    samples.reserve(n * S);
    ev.accept_rates_avg.assign(n, 0.0);
    for (size_t k = 0; k < S; ++k) {
      const std::vector<double> rates = engine_.StepSweep();
      for (size_t w = 0; w < n && w < rates.size(); ++w) ev.accept_rates_avg[w] += rates[w];
      EnergyAndHolesT<TenElemT> eh = model_.template CalEnergyAndHoles<false>(engine_.State(), comp);
      samples.insert(samples.end(), eh.energy.begin(), eh.energy.end());
    }
    for (auto &r : ev.accept_rates_avg) r /= double(S);
    const auto stat = MeanAndBinnedErrorSqrtNUniformBin(samples, n);
    ev.weight_sum = double(n * S);
    ev.e_loc_sum = stat.first * ev.weight_sum;
    ev.energy_error = stat.second;
    ReportLowAcceptance_(ev);                                                                  // :382
    return ev;
  }
  DeviceEvaluationT<TenElemT> operator()(ContractorT &contractor) { return Evaluate(contractor); }
  bool CollectsSRBuffers() const { return collect_sr_buffers_; }

 private:
  EngineT &engine_;
  Model &model_;
  const FermionDecoration *fermion_;
  const MonteCarloParams &params_;
  bool collect_sr_buffers_;
  static constexpr size_t kMaxAnomalyReports = 20;
  size_t reports_ = 0;
  void ReportLowAcceptance_(DeviceEvaluationT<TenElemT> &ev) {
    ev.low_acceptance_walkers = AcceptanceRateCheck(ev.accept_rates_avg);
    if (ev.low_acceptance_walkers.empty() || reports_++ >= kMaxAnomalyReports) return;
    const double mx = *std::max_element(ev.accept_rates_avg.begin(), ev.accept_rates_avg.end());
    for (const size_t w : ev.low_acceptance_walkers)
      std::cerr << "Walker " << w << ": Acceptance rate = " << ev.accept_rates_avg[w] << " is too small compared to the maximum over walkers "
                << mx << std::endl;
  }
};

// a model / updater pair that does not belong together: the U(1)xU(1) sector updater moves Hubbard states only; the transverse-field
// Ising model does not conserve S^z, so its chain needs the full-space updater; a fermionic model needs a decorated state
template <class MonteCarloSweepUpdater, class Model>
inline void CheckModelUpdaterPair(bool fermionic_state) {
  if (std::is_same<MonteCarloSweepUpdater, MCUpdateSquareNNHubbardU1U1OBC>::value && !std::is_same<Model, SquareHubbardModel>::value)
    throw std::invalid_argument("VMCPEPSOptimizer: MCUpdateSquareNNHubbardU1U1OBC belongs to SquareHubbardModel only");
  if (std::is_same<Model, TransverseFieldIsingSquareOBC>::value && !std::is_same<MonteCarloSweepUpdater, MCUpdateSquareNNFullSpaceUpdateOBC>::value)
    throw std::invalid_argument("VMCPEPSOptimizer: TransverseFieldIsingSquareOBC does not conserve S^z: it needs MCUpdateSquareNNFullSpaceUpdateOBC");
  if (IsFermionicModel<Model>::value != fermionic_state)
    throw std::invalid_argument("VMCPEPSOptimizer: a fermionic model needs a fermionic state (FermionDecoration), a bosonic model a bosonic one");
  if (fermionic_state && std::is_same<MonteCarloSweepUpdater, MCUpdateSquareNNFullSpaceUpdateOBC>::value)
    throw std::invalid_argument("VMCPEPSOptimizer: MCUpdateSquareNNFullSpaceUpdateOBC changes the particle number: not an updater of a fermionic model");
}

// VMCPEPSOptimizerParams (vmc_peps_optimizer_params.h): {OptimizerParams, MonteCarloParams, BMPSTruncateParams, tps_dump_base_name}.
// The reference hard-codes "./energy" for the trajectory; here the directory is a field with that default (empty: no CSV).
struct VMCPEPSOptimizerParams {
  OptimizerParams optimizer_params;
  MonteCarloParams mc_params;
  BMPSTruncateParams peps_params;
  std::string tps_dump_base_name;
  std::string energy_dump_dir = "./energy";
  VMCPEPSOptimizerParams(const OptimizerParams &opt, const MonteCarloParams &mc, const BMPSTruncateParams &trunc, const std::string &base = "")
      : optimizer_params(opt), mc_params(mc), peps_params(trunc), tps_dump_base_name(base) {}
  // no device call: run it before anything is built on the GPU
  void Validate(size_t n_walkers, size_t n_seeds) const {
    if (n_walkers == 0) throw std::invalid_argument("VMCPEPSOptimizerParams: at least one walker is required");
    if (mc_params.samples_per_walker == 0) throw std::invalid_argument("VMCPEPSOptimizerParams: samples_per_walker must be positive");
    if (n_seeds != n_walkers)
      throw std::invalid_argument("VMCPEPSOptimizerParams: " + std::to_string(n_seeds) + " seeds for " + std::to_string(n_walkers) +
                                  " walkers (one mt19937 engine per walker)");
    if (optimizer_params.IsAlgorithm<LBFGSParams>() &&
        optimizer_params.GetAlgorithmParams<LBFGSParams>().step_mode == LBFGSStepMode::kStrongWolfe)
      throw std::invalid_argument("VMCPEPSOptimizerParams: the strong-Wolfe line search on Monte-Carlo energies is not built (its trial "
                                  "evaluations are no iterations of the trajectory); use the fixed L-BFGS step");
    optimizer_params.ValidateGuards();             // the selector combinations and L-BFGS with rollback
  }
};

// VMCPEPSOptimizer (algorithm/vmc_update/vmc_peps_optimizer.h, vmc_peps_optimizer_impl.h:106-207, 470-542) on the resident state:
// Execute = WarmUp (normalises once) -> Optimizer::IterativeOptimize with MCEnergyGradEvaluator -> RefreshWavefunctionComponent +
// NormalizeStateOrder1 -> DumpData.  The caller builds the contractor, uploads the state and builds the component on it
// (TPSWaveFunctionComponentT::ResidentState), as for every class of this layer; the executor owns the Optimizer (pepsgpu_opt_begin
// adopts the uploaded state), the engine in resident mode and the evaluator.  tps_lowest_ / en_min_ (:118-121): whenever an
// evaluation's energy is below the minimum so far theta is copied device to device (pepsgpu_vmc_snapshot_save); the closing
// evaluation counts.  Spike recovery, the step selectors and checkpoints are the Optimizer's (OptimizerParams); the executor hands it
// the evaluator's energy-only variant for the selector trials and keeps its own trajectories and the lowest-state snapshot in
// on_evaluation_accepted, so an evaluation that spike recovery rejected is neither recorded nor ever "the lowest".  Not built: the
// JSONL log, more than one rank.
template <class MonteCarloSweepUpdater, class Model, typename TenElemT = double>
class VMCPEPSOptimizer {
 public:
  using ContractorT = BMPSContractorT<TenElemT>;
  using OptimizerT = Optimizer<TenElemT>;
  using Evaluator = typename OptimizerT::Evaluator;
  using EngineT = MonteCarloEngine<MonteCarloSweepUpdater, TenElemT>;
  // `phys_dim`: the components of the caller's state (fermions: the d stored ones; the contractor holds 4 d)
  VMCPEPSOptimizer(const VMCPEPSOptimizerParams &params, TPSWaveFunctionComponentT<TenElemT> &comp, MonteCarloSweepUpdater &updater,
                   Model &model, size_t n_seeds, size_t D, const ConfigurationRescueParams &rescue = ConfigurationRescueParams())
      : params_((params.Validate(comp.config.walkers(), n_seeds), CheckModelUpdaterPair<MonteCarloSweepUpdater, Model>(comp.fermion != nullptr),
                 params)),
        comp_(comp), D_(D), shape_(comp.contractor.rows(), comp.contractor.cols(), comp.contractor.phys_dim(), D),
        optimizer_(params_.optimizer_params, comp.contractor, comp.fermion),
        engine_(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), shape_, comp, params_.mc_params, updater, rescue),
        needs_sr_buffers_(params_.optimizer_params.template IsAlgorithm<StochasticReconfigurationParams>() ||
                          params_.optimizer_params.template IsAlgorithm<MinSRParams>()),
        evaluator_(engine_, model, params_.mc_params, needs_sr_buffers_, comp.fermion) {}

  void SetOptimizationCallback(const typename OptimizerT::OptimizationCallback &cb) { user_callback_ = cb; }
  void SetEnergyEvaluator(const Evaluator &ev) { custom_evaluator_ = ev; }
  // the evaluator of the step selectors' trials; with a custom evaluator and none given here the trials use the custom evaluator
  void SetEnergyOnlyEvaluator(const Evaluator &ev) { custom_energy_only_ = ev; }
  MCEnergyGradEvaluator<MonteCarloSweepUpdater, Model, TenElemT> &GetEvaluator() { return evaluator_; }

  // WarmUp + IterativeOptimize; theta is the state after the last step (not yet normalised)
  typename OptimizerT::OptimizationResult WarmUpAndOptimize() {
    engine_.WarmUp();                              // :108 (normalises once)
    energy_trajectory_.clear(); energy_error_traj_.clear(); grad_norm_.clear(); accept_rates_traj_.clear();
    en_min_ = std::numeric_limits<double>::max();
    has_lowest_ = false;
    timings_ = Timings();
    const auto t_begin = std::chrono::steady_clock::now();
    auto wrapped = [this](ContractorT &c) {
      const auto t0 = std::chrono::steady_clock::now();
      DeviceEvaluationT<TenElemT> ev = custom_evaluator_ ? custom_evaluator_(c) : evaluator_.Evaluate(c);
      timings_.evaluation_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();   // (ends in host read-backs)
      return ev;
    };
    Evaluator energy_only;
    if (custom_energy_only_ || !custom_evaluator_) energy_only = [this](ContractorT &c) {
      const auto t0 = std::chrono::steady_clock::now();
      DeviceEvaluationT<TenElemT> ev = custom_energy_only_ ? custom_energy_only_(c) : evaluator_.EvaluateEnergyOnly(c);
      timings_.evaluation_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      return ev;
    };
    // theta is still the evaluated state when an evaluation is accepted: the step comes after
    typename OptimizerT::OptimizationCallback cb = user_callback_;
    cb.on_evaluation_accepted = [this](const DeviceEvaluationT<TenElemT> &ev, const TenElemT &accepted_energy, size_t iter) {
      // the quotient of the sums, as before: the finished energy is the same real part and, for complex states, the same pair
      const TenElemT energy = ev.e_loc_sum / ev.weight_sum;
      (void)accepted_energy;
      energy_trajectory_.push_back(energy);
      energy_error_traj_.push_back(ev.energy_error);
      accept_rates_traj_.push_back(ev.accept_rates_avg);
      if (std::real(energy) < en_min_) {           // :118-121, in HBM
        en_min_ = std::real(energy);
        comp_.contractor.VMCSnapshotSave();
        has_lowest_ = true;
      }
      if (user_callback_.on_evaluation_accepted) user_callback_.on_evaluation_accepted(ev, accepted_energy, iter);
    };
    const auto t_opt = std::chrono::steady_clock::now();
    result_ = optimizer_.IterativeOptimize(wrapped, cb, energy_only);
    const auto t_end = std::chrono::steady_clock::now();
    timings_.optimize_s = std::chrono::duration<double>(t_end - t_opt).count();
    timings_.total_s = std::chrono::duration<double>(t_end - t_begin).count();
    grad_norm_ = result_.gradient_norms;
    return result_;
  }
  // :202-203
  void FinalizeState() {
    engine_.RefreshWavefunctionComponent();
    engine_.NormalizeStateOrder1();
  }
  void Execute() {
    const auto t0 = std::chrono::steady_clock::now();
    WarmUpAndOptimize();
    FinalizeState();
    DumpData();
    timings_.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  // host-clock seconds of the last run: inside the evaluator (sampling), inside IterativeOptimize (sampling + finish / clip / step) and
  // in all (warm-up, closing normalisation and dumps included); every part ends in a call that synchronises the stream
  struct Timings { double evaluation_s = 0.0, optimize_s = 0.0, total_s = 0.0; };
  const Timings &GetTimings() const { return timings_; }

  SplitIndexTPST<TenElemT> GetState() const { return optimizer_.GetState(shape_.rows(), shape_.cols(), StoredPhysDim(), D_); }
  // the parameters of the lowest energy as they were when it was evaluated (not rescaled by the closing normalisation)
  SplitIndexTPST<TenElemT> GetLowestState() const {
    if (!has_lowest_) throw std::logic_error("VMCPEPSOptimizer::GetLowestState: no evaluation yet");
    SplitIndexTPST<TenElemT> ext(shape_.rows(), shape_.cols(), shape_.PhysicalDim(), D_);
    comp_.contractor.VMCSnapshotRead(ext);
    if (!comp_.fermion) return ext;
    SplitIndexTPST<TenElemT> s(shape_.rows(), shape_.cols(), StoredPhysDim(), D_);      // variant 0 = the stored arrays
    for (size_t r = 0; r < s.rows(); ++r)
      for (size_t c = 0; c < s.cols(); ++c)
        for (size_t k = 0; k < s.PhysicalDim(); ++k) std::copy(ext.component(r, c, k), ext.component(r, c, k) + ext.slot(), s.component(r, c, k));
    return s;
  }
  double GetMinEnergy() const { return en_min_; }
  TenElemT GetCurrentEnergy() const { return energy_trajectory_.empty() ? TenElemT(0.0) : energy_trajectory_.back(); }
  const std::vector<TenElemT> &GetEnergyTrajectory() const { return energy_trajectory_; }
  const std::vector<double> &GetEnergyErrorTrajectory() const { return energy_error_traj_; }
  const std::vector<double> &GetGradientNormTrajectory() const { return grad_norm_; }
  const std::vector<std::vector<double>> &GetAcceptRatesTrajectory() const { return accept_rates_traj_; }
  const typename OptimizerT::OptimizationResult &GetResult() const { return result_; }
  const SpikeStatistics &GetSpikeStatistics() const { return result_.spike_stats; }
  OptimizerT &GetOptimizer() { return optimizer_; }
  EngineT &GetEngine() { return engine_; }

  void DumpData() const { DumpData(params_.tps_dump_base_name, params_.energy_dump_dir); }
  // :512-542: base + "final" / base + "lowest" (nothing when base is empty), the walkers' configurations to config_dump_path
  // (configuration<walker>, empty: no dump), <energy_dir>/energy_trajectory.csv (empty: no CSV)
  void DumpData(const std::string &tps_base_name, const std::string &energy_dir = "./energy") const {
    if (!tps_base_name.empty()) {
      EnsureDirectoryExists(tps_base_name + "final");
      GetState().Dump(tps_base_name + "final");
      if (has_lowest_) {
        EnsureDirectoryExists(tps_base_name + "lowest");
        GetLowestState().Dump(tps_base_name + "lowest");
      }
    }
    if (!params_.mc_params.config_dump_path.empty())
      for (size_t w = 0; w < comp_.config.walkers(); ++w) DumpConfiguration(comp_.config, w, params_.mc_params.config_dump_path, w);
    if (!energy_dir.empty()) {
      EnsureDirectoryExists(energy_dir);
      WriteEnergyTrajectoryCsv_(energy_dir + "/energy_trajectory.csv");
    }
  }

 private:
  size_t StoredPhysDim() const { return comp_.fermion ? comp_.fermion->d() : shape_.PhysicalDim(); }
  void WriteEnergyTrajectoryCsv_(const std::string &csv_path) const {      // :475-501
    std::ofstream csv(csv_path);
    if (!csv) throw std::ios_base::failure("VMCPEPSOptimizer: failed to open " + csv_path);
    csv << "iteration,energy,energy_error,gradient_norm\n";
    for (size_t i = 0; i < energy_trajectory_.size(); ++i) {
      const double err = i < energy_error_traj_.size() ? energy_error_traj_[i] : 0.0, gnorm = i < grad_norm_.size() ? grad_norm_[i] : 0.0;
      csv << i << "," << std::setprecision(17) << std::real(energy_trajectory_[i]) << "," << err << "," << gnorm << "\n";
    }
    if (!csv) throw std::ios_base::failure("VMCPEPSOptimizer: failed to write " + csv_path);
  }
  VMCPEPSOptimizerParams params_;
  TPSWaveFunctionComponentT<TenElemT> &comp_;
  size_t D_;
  SplitIndexTPST<TenElemT> shape_;                 // extents only
  OptimizerT optimizer_;
  EngineT engine_;
  bool needs_sr_buffers_;
  MCEnergyGradEvaluator<MonteCarloSweepUpdater, Model, TenElemT> evaluator_;
  Evaluator custom_evaluator_, custom_energy_only_;
  typename OptimizerT::OptimizationCallback user_callback_;
  typename OptimizerT::OptimizationResult result_;
  std::vector<TenElemT> energy_trajectory_;
  std::vector<double> energy_error_traj_, grad_norm_;
  std::vector<std::vector<double>> accept_rates_traj_;
  double en_min_ = std::numeric_limits<double>::max();
  bool has_lowest_ = false;
  Timings timings_;
};

}  // namespace qlpeps_gpu
