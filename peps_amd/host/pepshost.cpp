// C shim over the C++ host layer (qlpeps_gpu.h) so that the Python tests / bench drive exactly the
// host code a reference user would compile (updaters, solvers, evaluators), not a re-implementation.
#include <cstring>
#include <memory>

#include "qlpeps_gpu.h"

using namespace qlpeps_gpu;

namespace {
thread_local std::string g_err;
// GPU of the contractors built below: one rank per GPU -> LOCAL_RANK unless pepshost_set_device says otherwise
int default_device() {
  const char *e = getenv("LOCAL_RANK");
  return e ? atoi(e) : 0;
}
int g_device = default_device();

template <typename F>
int guarded(F &&f) {
  try {
    f();
    return 0;
  } catch (const std::invalid_argument &e) { g_err = e.what(); return PEPSGPU_EINVAL;
  } catch (const std::out_of_range &e) { g_err = e.what(); return PEPSGPU_ERANGE;
  } catch (const std::logic_error &e) { g_err = e.what(); return PEPSGPU_ESTATE;
  } catch (const std::exception &e) { g_err = e.what(); return PEPSGPU_EEMPTY; }
}

SplitIndexTPS make_state(int rows, int cols, int D, int d, const double *flat) {
  SplitIndexTPS s(rows, cols, d, D);
  std::copy(flat, flat + s.flat().size(), s.flat().begin());
  return s;
}
// element-type generic form: `flat` = doubles, interleaved (re, im) pairs for QLTEN_Complex
template <typename TenElemT>
SplitIndexTPST<TenElemT> make_state_t(int rows, int cols, int D, int d, const double *flat) {
  SplitIndexTPST<TenElemT> s(rows, cols, d, D);
  const TenElemT *src = reinterpret_cast<const TenElemT *>(flat);
  std::copy(src, src + s.flat().size(), s.flat().begin());
  return s;
}
template <typename TenElemT>
void copy_out(const std::vector<TenElemT> &v, double *out) {
  if (out) std::copy(dptr(v.data()), dptr(v.data()) + v.size() * (ElemTraits<TenElemT>::is_complex ? 2 : 1), out);
}
// BMPSTruncateParams of the contractors built below: SVD(chi, chi, 0) unless pepshost_set_truncate_params changed
// D_min / trunc_err / scheme (D_max is always the call's chi)
struct TruncOverride { int d_min = -1; double trunc_err = 0.0; int scheme = 0; double tol = 0.0; int iters = 0; } g_trunc;
BMPSTruncateParams trunc_params(int chi) {
  const size_t dmin = g_trunc.d_min < 0 ? (size_t)chi : (size_t)std::min(g_trunc.d_min, chi);
  if (g_trunc.scheme == 1) return BMPSTruncateParams::Variational2Site(dmin, chi, g_trunc.trunc_err, g_trunc.tol, g_trunc.iters);
  if (g_trunc.scheme == 2) return BMPSTruncateParams::Variational1Site(dmin, chi, g_trunc.trunc_err, g_trunc.tol, g_trunc.iters);
  return BMPSTruncateParams::SVD(dmin, chi, g_trunc.trunc_err);
}
Configuration make_cfg(int n, int rows, int cols, const int32_t *cfg) {
  Configuration c(n, rows, cols);
  std::copy(cfg, cfg + (size_t)n * rows * cols, c.data());
  return c;
}

// ---- element-type generic bodies of the entry points below (TenElemT = QLTEN_Double / QLTEN_Complex) ----
template <typename TenElemT>
void energy_and_holes_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n,
                           const int32_t *configs, int model, const double *p, double *amplitudes_out,
                           double *energies_out, double *holes_out, double *psi_out, int *n_psi_out) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor);
  EnergyAndHolesT<TenElemT> eh;
  if (model == 0) {
    SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]);
    eh = holes_out ? m.CalEnergyAndHoles<true>(sitps, comp) : m.CalEnergyAndHoles<false>(sitps, comp);
  } else if (model == 2) {
    SquareSpinOneHalfJ1J2XXZModelOBC m(p[0], p[1], p[2], p[3], p[4]);
    eh = holes_out ? m.CalEnergyAndHoles<true>(sitps, comp) : m.CalEnergyAndHoles<false>(sitps, comp);
  } else if (model == 3) {
    SpinOneHalfTriHeisenbergSqrPEPS m;
    eh = holes_out ? m.CalEnergyAndHoles<true>(sitps, comp) : m.CalEnergyAndHoles<false>(sitps, comp);
  } else if (model == 4) {
    SpinOneHalfTriJ1J2HeisenbergSqrPEPS m(p[0]);
    eh = holes_out ? m.CalEnergyAndHoles<true>(sitps, comp) : m.CalEnergyAndHoles<false>(sitps, comp);
  } else {
    TransverseFieldIsingSquareOBC m(p[0]);
    eh = holes_out ? m.CalEnergyAndHoles<true>(sitps, comp) : m.CalEnergyAndHoles<false>(sitps, comp);
  }
  constexpr int z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  copy_out(comp.amplitude, amplitudes_out);
  copy_out(eh.energy, energies_out);
  copy_out(eh.holes, holes_out);
  if (n_psi_out) *n_psi_out = (int)eh.psi_list.size();
  if (psi_out)
    for (size_t k = 0; k < eh.psi_list.size(); ++k) copy_out(eh.psi_list[k], psi_out + k * n * z);
}

template <typename TenElemT>
void exact_sum_partial_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat,
                            const int32_t *all_configs, int n_configs, int model, const double *p, int rank, int size,
                            int batch, double *packed_out) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  std::vector<double> packed;
  auto capture = [&](std::vector<double> &v) { packed = v; };
  if (model == 0) {
    SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  } else if (model == 2) {
    SquareSpinOneHalfJ1J2XXZModelOBC m(p[0], p[1], p[2], p[3], p[4]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  } else if (model == 3) {
    SpinOneHalfTriHeisenbergSqrPEPS m;
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  } else if (model == 4) {
    SpinOneHalfTriJ1J2HeisenbergSqrPEPS m(p[0]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  } else {
    TransverseFieldIsingSquareOBC m(p[0]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  }
  std::copy(packed.begin(), packed.end(), packed_out);
}

// Optimizer::IterativeOptimize with the exact-summation evaluator, the whole loop in one call: the state is uploaded once, every
// iteration evaluates the device-resident state, finishes the gradient, clips and steps in HBM; the state comes back once at the end.
// rule 0 SGD (momentum, nesterov, weight_decay), 1 AdaGrad (epsilon, initial_accumulator_value), 2 Adam (beta1, beta2, epsilon,
// weight_decay).  energies_out: iterations + 1 entries (re [, im]); grad_norms_out (nullable): the same count.
template <typename TenElemT>
void optimize_exact_sum_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, const int32_t *all_configs,
                             int n_configs, int model, const double *p, int rule, double lr, const double *rule_params, int n_rule_params,
                             int iterations, double clip_value, double clip_norm, int batch, double *energies_out, double *grad_norms_out,
                             double *state_out) {
  if (iterations < 0 || n_configs < 1 || batch < 1) throw std::invalid_argument("pepshost_optimize_exact_sum: bad iterations / n_configs / batch");
  if (model < 0 || model > 4) throw std::invalid_argument("pepshost_optimize_exact_sum: model must be xxz, tfim, j1j2, triangle or trij1j2");
  static const int want[3] = {3, 2, 4};
  if (rule < 0 || rule > 2 || n_rule_params != want[rule] || !rule_params)
    throw std::invalid_argument("pepshost_optimize_exact_sum: rule 0 SGD (3 parameters), 1 AdaGrad (2), 2 Adam (4)");
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  OptimizerParams::BaseParams base((size_t)iterations, 0.0, 0.0, (size_t)iterations + 1, lr);   // the stopping criteria are off
  if (clip_value > 0.0) base.clip_value = clip_value;
  if (clip_norm > 0.0) base.clip_norm = clip_norm;
  const double *q = rule_params;
  AlgorithmParams algo = rule == 0   ? AlgorithmParams(SGDParams(q[0], q[1] != 0.0, q[2]))
                         : rule == 1 ? AlgorithmParams(AdaGradParams(q[0], q[1]))
                                     : AlgorithmParams(AdamParams(q[0], q[1], q[2], q[3]));
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(base, algo), contractor);
  auto run = [&](auto &m) {
    return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) { return ExactSumAccumulateResident(sitps, all, c, m, (size_t)batch); });
  };
  typename Optimizer<TenElemT>::OptimizationResult res;
  if (model == 0) { SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]); res = run(m); }
  else if (model == 2) { SquareSpinOneHalfJ1J2XXZModelOBC m(p[0], p[1], p[2], p[3], p[4]); res = run(m); }
  else if (model == 3) { SpinOneHalfTriHeisenbergSqrPEPS m; res = run(m); }
  else if (model == 4) { SpinOneHalfTriJ1J2HeisenbergSqrPEPS m(p[0]); res = run(m); }
  else { TransverseFieldIsingSquareOBC m(p[0]); res = run(m); }
  copy_out(res.energy_trajectory, energies_out);
  if (grad_norms_out) std::copy(res.gradient_norms.begin(), res.gradient_norms.end(), grad_norms_out);
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
}

// One SR iteration of Optimizer::IterativeOptimize on a given sample set (weight 1 per sample, no sampling): evaluate, finish, natural
// gradient on the device, theta -= lr x, closing evaluation.  info_out = [E before, E after, CG iterations, |x|, CG residual norm]
// (energies: real parts).  TFIM and XXZ models.
template <typename TenElemT>
void sr_step_samples_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, const int32_t *configs,
                          int model, const double *p, double lr, double diag_shift, int cg_max_iter, double cg_relative_tolerance,
                          int normalize_update, double *state_out, double *info_out) {
  if (model != 0 && model != 1) throw std::invalid_argument("pepshost_sr_step_samples: model must be xxz or tfim");
  if (n < 1 || cg_max_iter < 0) throw std::invalid_argument("pepshost_sr_step_samples: bad sample count / CG iterations");
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
  const Configuration samples = make_cfg(n, rows, cols, configs);
  StochasticReconfigurationParams sr;
  sr.cg_params.max_iter = (size_t)cg_max_iter;
  sr.cg_params.relative_tolerance = cg_relative_tolerance;
  sr.diag_shift = diag_shift;
  sr.normalize_update = normalize_update != 0;
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(OptimizerParams::BaseParams(1, 0.0, 0.0, 2, lr), sr), contractor);
  typename Optimizer<TenElemT>::OptimizationResult res;
  auto run = [&](auto &m) {
    return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) { return SampleSetAccumulateResident(sitps, samples, c, m); });
  };
  if (model == 0) { SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]); res = run(m); }
  else { TransverseFieldIsingSquareOBC m(p[0]); res = run(m); }
  info_out[0] = std::real(res.energy_trajectory.at(0)); info_out[1] = std::real(res.energy_trajectory.at(1));
  info_out[2] = (double)res.sr_iterations; info_out[3] = res.sr_natural_grad_norm; info_out[4] = res.sr_residual_norm;
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
}

// The MinSR twin of sr_step_samples_impl: one iteration of Optimizer::IterativeOptimize with MinSRParams on a given sample set.
// info_out = [E before, E after, |x|, max eigenvalue of T, cutoff, eigenvalues kept, Jacobi sweeps].  exact_sum != 0 evaluates by exact
// summation over `configs` instead: that evaluator keeps no sample set, so the MinSR update refuses (std::invalid_argument).
template <typename TenElemT>
void minsr_step_samples_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, const int32_t *configs,
                             int model, const double *p, double lr, double r_pinv, double a_pinv, int soft_cutoff, int exact_sum,
                             double *state_out, double *info_out) {
  if (model != 0 && model != 1) throw std::invalid_argument("pepshost_minsr_step_samples: model must be xxz or tfim");
  if (n < 1) throw std::invalid_argument("pepshost_minsr_step_samples: bad sample count");
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
  const Configuration samples = make_cfg(n, rows, cols, configs);
  std::vector<std::vector<int32_t>> all(exact_sum ? n : 0);
  for (size_t i = 0; i < all.size(); ++i) all[i].assign(configs + i * rows * cols, configs + (i + 1) * rows * cols);
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(OptimizerParams::BaseParams(1, 0.0, 0.0, 2, lr), MinSRParams(r_pinv, a_pinv, soft_cutoff != 0)),
                          contractor);
  typename Optimizer<TenElemT>::OptimizationResult res;
  auto run = [&](auto &m) {
    return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) {
      return exact_sum ? ExactSumAccumulateResident(sitps, all, c, m, (size_t)n) : SampleSetAccumulateResident(sitps, samples, c, m);
    });
  };
  if (model == 0) { SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]); res = run(m); }
  else { TransverseFieldIsingSquareOBC m(p[0]); res = run(m); }
  const auto &mi = opt.LastMinSRInfo();
  info_out[0] = std::real(res.energy_trajectory.at(0)); info_out[1] = std::real(res.energy_trajectory.at(1));
  info_out[2] = res.sr_natural_grad_norm; info_out[3] = mi.lambda_max; info_out[4] = mi.cutoff;
  info_out[5] = (double)mi.n_kept; info_out[6] = (double)mi.sweeps;
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
}

template <typename TenElemT>
void mc_energy_grad_partial_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n,
                                 int32_t *configs, const uint64_t *seeds, int updater, int model, const double *p,
                                 int warmup_sweeps, int n_samples, double *packed_out, double *accept_out) {
  if (model < 0 || model > 4) throw std::invalid_argument("pepshost_mc_energy_grad_partial: model must be xxz, tfim, j1j2, triangle or trij1j2");
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor);
  std::vector<uint64_t> sd(seeds, seeds + n);
  MCUpdateSquareNNExchangeOBC ex(sd);
  MCUpdateSquareNNFullSpaceUpdateOBC fs(sd);
  MCUpdateSquareTNN3SiteExchange t3(sd);
  std::vector<double> rates, acc_rate(n, 0.0);
  auto sweep = [&]() {
    if (updater == 0) ex(sitps, comp, rates);
    else if (updater == 2) t3(sitps, comp, rates);
    else fs(sitps, comp, rates);
  };
  for (int s = 0; s < warmup_sweeps; ++s) sweep();
  SquareSpinOneHalfXXZModelOBC xxz(p[0], p[1], p[2]);
  SquareSpinOneHalfJ1J2XXZModelOBC j1j2(p[0], p[1], p[2], p[3], p[4]);
  TransverseFieldIsingSquareOBC tfim(p[0]);
  SpinOneHalfTriHeisenbergSqrPEPS tri;
  SpinOneHalfTriJ1J2HeisenbergSqrPEPS trij1j2(p[0]);
  GradAccumulatorT<TenElemT> acc(sitps);
  contractor.GradReset();
  for (int k = 0; k < n_samples; ++k) {
    sweep();
    for (int w = 0; w < n; ++w) acc_rate[w] += rates[w];
    EnergyAndHolesT<TenElemT> eh = model == 0   ? xxz.CalEnergyAndHoles<true>(sitps, comp, true)
                                   : model == 2 ? j1j2.CalEnergyAndHoles<true>(sitps, comp, true)
                                   : model == 3 ? tri.CalEnergyAndHoles<true>(sitps, comp, true)
                                   : model == 4 ? trij1j2.CalEnergyAndHoles<true>(sitps, comp, true)
                                                : tfim.CalEnergyAndHoles<true>(sitps, comp, true);
    acc.AccumulateDevice(comp, eh, false);
  }
  if (n_samples > 0) acc.FetchDevice(contractor);
  std::vector<double> packed = acc.Pack();
  std::copy(packed.begin(), packed.end(), packed_out);
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
  if (accept_out) for (int w = 0; w < n; ++w) accept_out[w] = n_samples ? acc_rate[w] / n_samples : 0.0;
}

template <typename TenElemT>
void mc_sweeps_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n,
                    int32_t *configs, const uint64_t *seeds, int updater, int n_sweeps, double *amplitudes_out,
                    double *accept_rates_out) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor);
  std::vector<uint64_t> sd(seeds, seeds + n);
  std::vector<double> rates, acc(n, 0.0);
  if (updater == 0) {
    MCUpdateSquareNNExchangeOBC upd(sd);
    for (int s = 0; s < n_sweeps; ++s) { upd(sitps, comp, rates); for (int w = 0; w < n; ++w) acc[w] += rates[w]; }
  } else if (updater == 2) {
    MCUpdateSquareTNN3SiteExchange upd(sd);
    for (int s = 0; s < n_sweeps; ++s) { upd(sitps, comp, rates); for (int w = 0; w < n; ++w) acc[w] += rates[w]; }
  } else {
    MCUpdateSquareNNFullSpaceUpdateOBC upd(sd);
    for (int s = 0; s < n_sweeps; ++s) { upd(sitps, comp, rates); for (int w = 0; w < n; ++w) acc[w] += rates[w]; }
  }
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
  copy_out(comp.amplitude, amplitudes_out);
  for (int w = 0; w < n; ++w) accept_rates_out[w] = n_sweeps ? acc[w] / n_sweeps : 0.0;
}
template <typename TenElemT>
void measure_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, int32_t *configs,
                  const uint64_t *seeds, int updater, int model, const double *p, int warmup_sweeps, int n_samples,
                  int sweeps_between_samples, const char *dump_dir, char *keys_out, int keys_cap, double *values_out,
                  long values_cap, long *values_len) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor);
  SquareSpinOneHalfXXZModelOBC xxz(p[0], p[1], p[2]);
  SquareSpinOneHalfJ1J2XXZModelOBC j1j2(p[0], p[1], p[2], p[3], p[4]);
  SpinOneHalfTriHeisenbergSqrPEPS tri;
  SpinOneHalfTriJ1J2HeisenbergSqrPEPS trij(p[0]);
  TransverseFieldIsingSquareOBC tfim(p[0]);
  if (model < 0 || model > 4) throw std::invalid_argument("pepshost_measure: model must be xxz, tfim, j1j2, triangle or trij1j2");
  xxz.SetEnableStructureFactor(p[7] != 0.0);                  // params[7]: structure factor switch (xxz only)
  xxz.SetStructureFactorReferenceStackState(p[6] != 0.0);     // params[6]: the DOWN stack as the reference's traversal leaves it (K8; off)
  std::string keys;
  std::vector<double> vals;                                   // QLTEN_Complex: every number as a (re, im) pair
  auto push = [&](const auto &v) {
    vals.push_back(std::real(v));
    if constexpr (ElemTraits<TenElemT>::is_complex) vals.push_back(std::imag(v));
  };
  auto emit = [&](const std::string &key, const std::vector<TenElemT> &a, const std::vector<double> *b, size_t len) {
    keys += key + ":" + std::to_string(len) + ";";
    for (const auto &v : a) push(v);
    if (b) {
      if (b->empty()) for (size_t k = 0; k < a.size(); ++k) push(0.0);
      else for (double v : *b) push(v);
    }
  };
  PsiSummaryT<TenElemT> psi;
  if (n_samples <= 0) {
    ObservableMapT<TenElemT> obs = model == 0   ? xxz.EvaluateObservables(sitps, comp)
                                   : model == 1 ? tfim.EvaluateObservables(sitps, comp)
                                   : model == 2 ? j1j2.EvaluateObservables(sitps, comp)
                                   : model == 3 ? tri.EvaluateObservables(sitps, comp)
                                                : trij.EvaluateObservables(sitps, comp);
    for (const auto &kv : obs.values) emit(kv.first, kv.second, nullptr, obs.len(kv.first));
    psi = model == 0   ? xxz.SquareNNModelMeasurementSolver<SquareSpinOneHalfXXZModelOBC>::template EvaluatePsiSummaryT<TenElemT>()
          : model == 1 ? tfim.template EvaluatePsiSummaryT<TenElemT>()
          : model == 2 ? j1j2.SquareNNNModelMeasurementSolver<SquareSpinOneHalfJ1J2XXZModelOBC>::template EvaluatePsiSummaryT<TenElemT>()
          : model == 3 ? tri.SquareNNNModelMeasurementSolver<SpinOneHalfTriHeisenbergSqrPEPS>::template EvaluatePsiSummaryT<TenElemT>()
                       : trij.template EvaluatePsiSummaryT<TenElemT>();
  } else {
    std::vector<uint64_t> sd(seeds, seeds + n);
    MCMeasurementParams mp;
    mp.num_samples = n_samples; mp.num_warmup_sweeps = warmup_sweeps; mp.sweeps_between_samples = sweeps_between_samples;
    auto run = [&](auto &upd, auto &solver) {
      MCPEPSMeasurer<std::decay_t<decltype(upd)>, std::decay_t<decltype(solver)>, TenElemT> m(sitps, comp, mp, upd, solver);
      m.Execute();
      if (dump_dir && dump_dir[0]) m.DumpData(dump_dir);
      for (const auto &kv : m.ObservableRegistry()) emit(kv.first, kv.second.first, &kv.second.second, kv.second.first.size());
      psi.psi_mean.assign(n, TenElemT(0.0)); psi.psi_rel_err.assign(n, 0.0);
      for (int w = 0; w < n; ++w) { psi.psi_mean[w] = m.PsiSamples().back()[w].first; psi.psi_rel_err[w] = m.PsiSamples().back()[w].second; }
    };
    MCUpdateSquareNNExchangeOBC ex(sd);
    MCUpdateSquareNNFullSpaceUpdateOBC fs(sd);
    MCUpdateSquareTNN3SiteExchange t3(sd);
    if (updater == 0 && model == 0) run(ex, xxz);
    else if (updater == 0 && model == 1) run(ex, tfim);
    else if (updater == 0 && model == 2) run(ex, j1j2);
    else if (updater == 0 && model == 3) run(ex, tri);
    else if (updater == 0) run(ex, trij);
    else if (updater == 2 && model == 0) run(t3, xxz);
    else if (updater == 2 && model == 1) run(t3, tfim);
    else if (updater == 2 && model == 2) run(t3, j1j2);
    else if (updater == 2 && model == 3) run(t3, tri);
    else if (updater == 2) run(t3, trij);
    else if (model == 0) run(fs, xxz);
    else if (model == 1) run(fs, tfim);
    else if (model == 2) run(fs, j1j2);
    else if (model == 3) run(fs, tri);
    else run(fs, trij);
    std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
  }
  for (const auto &v : psi.psi_mean) push(v);
  for (double v : psi.psi_rel_err) push(v);
  if ((int)keys.size() + 1 > keys_cap || (long)vals.size() > values_cap) throw std::out_of_range("pepshost_measure: output buffer too small");
  std::copy(keys.begin(), keys.end(), keys_out);
  keys_out[keys.size()] = 0;
  std::copy(vals.begin(), vals.end(), values_out);
  *values_len = (long)vals.size();
}
template <typename TenElemT>
void exact_sum_measure_partial_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat,
                                    const int32_t *all_configs, int n_configs, int model, const double *p, int rank, int size,
                                    int batch, char *keys_out, int keys_cap, double *values_out, long values_cap, long *values_len) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all;
  if (n_configs >= 0) {
    all.resize(n_configs);
    for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  } else {
    all = GenerateAllBinaryConfigs(cols, rows);
  }
  if (model != 0 && model != 1 && model != 2) throw std::invalid_argument("pepshost_exact_sum_measure_partial: model must be xxz, tfim or j1j2");
  if (!all.empty() && (size_t)rank >= all.size()) {           // a rank without configurations contributes nothing
    if (keys_cap < 1 || values_cap < 1) throw std::out_of_range("pepshost_exact_sum_measure_partial: output buffer too small");
    keys_out[0] = 0; values_out[0] = 0.0; *values_len = 1;
    return;
  }
  std::vector<double> packed;
  auto capture = [&](std::vector<double> &v) { packed = v; v[0] = 1.0; };   // keep the raw sums; normalise in the caller
  std::map<std::string, std::vector<TenElemT>> res;
  if (model == 0) {
    SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]);
    m.SetEnableStructureFactor(p[7] != 0.0);
    res = ExactSumMeasurer(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  } else if (model == 1) {
    TransverseFieldIsingSquareOBC m(p[0]);
    res = ExactSumMeasurer(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  } else {
    SquareSpinOneHalfJ1J2XXZModelOBC m(p[0], p[1], p[2], p[3], p[4]);
    res = ExactSumMeasurer(sitps, all, contractor, m, rank, size, (size_t)batch, capture);
  }
  std::string keys;
  for (const auto &kv : res) keys += kv.first + ":" + std::to_string(kv.second.size()) + ";";
  if ((int)keys.size() + 1 > keys_cap || (long)packed.size() > values_cap) throw std::out_of_range("pepshost_exact_sum_measure_partial: output buffer too small");
  std::copy(keys.begin(), keys.end(), keys_out);
  keys_out[keys.size()] = 0;
  std::copy(packed.begin(), packed.end(), values_out);
  *values_len = (long)packed.size();
}

// ---- fermionic entry points, element-type generic (sitps_ext_flat: 4 d sign-decorated components per site) ----
template <typename TenElemT>
void fermion_energy_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                         const double *sitps_ext_flat, int n, const int32_t *configs, int model, const double *prm,
                         double *amplitudes_out, double *energies_out, double *psi_out, int *n_psi_out, int n_prm = 4) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor, &dec);
  copy_out(comp.amplitude, amplitudes_out);
  EnergyAndHolesT<TenElemT> eh;
  if (model == 0) {
    SquareSpinlessFermion m(prm[0], prm[2], prm[1]);      // (t, t2, V): params = [t, V, t2, -]
    eh = m.CalEnergyAndHoles<false>(sitps, comp);
  } else if (model == 3) {
    SquareHubbardModel m(prm[0], prm[1], prm[2]);         // [t, U, mu]
    eh = m.CalEnergyAndHoles<false>(sitps, comp);
  } else {
    SquaretJVModel m(prm[0], n_prm > 4 ? prm[4] : 0.0, prm[1], prm[2], prm[3]);      // [t, J, V, mu, (t2)]
    eh = m.CalEnergyAndHoles<false>(sitps, comp);
  }
  constexpr int z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  copy_out(eh.energy, energies_out);
  if (n_psi_out) *n_psi_out = (int)eh.psi_list.size();
  if (psi_out)
    for (size_t k = 0; k < eh.psi_list.size(); ++k) copy_out(eh.psi_list[k], psi_out + k * n * z);
}

template <typename TenElemT>
void fermion_exact_sum_partial_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                    const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, double t,
                                    double V, int rank, int size, int batch, double *packed_out) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  std::vector<double> packed;
  auto capture = [&](std::vector<double> &v) { packed = v; };
  SquareSpinlessFermion m(t, V);
  ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture, &dec);
  std::copy(packed.begin(), packed.end(), packed_out);
}
// ... with the model chosen as fermion_energy_impl chooses it: 0 SquareSpinlessFermion [t, V, t2, -], 1 SquaretJVModel [t, J, V, mu, (t2)]
template <typename TenElemT>
void fermion_exact_sum_partial_prm_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                        const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model,
                                        const double *prm, int n_prm, int rank, int size, int batch, double *packed_out) {
  if ((model != 0 && model != 1 && model != 3) || !prm || n_prm < (model == 3 ? 3 : 4))
    throw std::invalid_argument("pepshost_fermion_exact_sum_partial_prm: model 0 / 1 with at least four parameters, or 3 (hubbard) with three");
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  std::vector<double> packed;
  auto capture = [&](std::vector<double> &v) { packed = v; };
  if (model == 0) {
    SquareSpinlessFermion m(prm[0], prm[2], prm[1]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture, &dec);
  } else if (model == 3) {
    SquareHubbardModel m(prm[0], prm[1], prm[2]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture, &dec);
  } else {
    SquaretJVModel m(prm[0], n_prm > 4 ? prm[4] : 0.0, prm[1], prm[2], prm[3]);
    ExactSumEnergyEvaluator(sitps, all, contractor, m, rank, size, (size_t)batch, capture, &dec);
  }
  std::copy(packed.begin(), packed.end(), packed_out);
}

template <typename TenElemT>
void fermion_mc_sweeps_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                            const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int n_sweeps,
                            double *amplitudes_out, double *accept_out, int updater = 0) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor, &dec);
  std::vector<uint64_t> sd(seeds, seeds + n);
  MCUpdateSquareNNExchangeOBC ex(sd);
  MCUpdateSquareTNN3SiteExchange t3(sd);
  MCUpdateSquareNNHubbardU1U1OBC hub(sd);
  std::vector<double> rates, acc(n, 0.0);
  for (int s = 0; s < n_sweeps; ++s) {
    if (updater == 2) t3(sitps, comp, rates);
    else if (updater == 3) hub(sitps, comp, rates);
    else ex(sitps, comp, rates);
    for (int w = 0; w < n; ++w) acc[w] += rates[w];
  }
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
  copy_out(comp.amplitude, amplitudes_out);
  if (accept_out) for (int w = 0; w < n; ++w) accept_out[w] = n_sweeps ? acc[w] / n_sweeps : 0.0;
}

template <typename TenElemT>
void fermion_measure_energy_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                 const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int warmup_sweeps,
                                 int n_samples, int sweeps_between, int model, const double *prm, double *energies_out,
                                 double *accept_out, int n_prm = 4) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor, &dec);
  std::vector<uint64_t> sd(seeds, seeds + n);
  MCUpdateSquareNNExchangeOBC ex(sd);
  std::vector<double> rates, acc(n, 0.0);
  for (int s = 0; s < warmup_sweeps; ++s) ex(sitps, comp, rates);
  comp.SetOrder(ROW_MAJOR);
  comp.EvaluateAmplitude();                                  // NormalizeStateOrder1: tps_sample_ = WaveFunctionComponentT(...) (:235-236)
  SquareSpinlessFermion spinless(prm[0], prm[2], prm[1]);     // model 0: (t, t2, V) from [t, V, t2, -]
  SquaretJVModel tj(prm[0], n_prm > 4 ? prm[4] : 0.0, prm[1], prm[2], prm[3]);     // model 1: [t, J, V, mu, (t2)]
  constexpr int z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  for (int k = 0; k < n_samples; ++k) {
    for (int s = 0; s < sweeps_between; ++s) {
      ex(sitps, comp, rates);
      for (int w = 0; w < n; ++w) acc[w] += rates[w];
    }
    EnergyAndHolesT<TenElemT> eh = model == 0 ? spinless.CalEnergyAndHoles<false>(sitps, comp) : tj.CalEnergyAndHoles<false>(sitps, comp);
    copy_out(eh.energy, energies_out + (size_t)k * n * z);
  }
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
  const int total = std::max(1, n_samples * sweeps_between);
  if (accept_out) for (int w = 0; w < n; ++w) accept_out[w] = acc[w] / total;
}
// ---- the measurement solvers of the fermionic models.  model 0: SquareSpinlessFermion [t, V, t2]; 1: SquaretJVModel [t, J, V, mu, t2];
// 2: SquaretJNNModel [t, J, mu] (the nearest-neighbour form: no diagonal-bond keys); 3: SquareHubbardModel [t, U, mu] (with
// double_occupancy).  Output in the format of pepshost_measure: keys
// "key:len;", every number of a complex state as a (re, im) pair. ----
// SC_singlet_pair_corr of the t-J models (SingletPairCorrelationMixin): the switch and the selected reference bonds [n_bonds][2] = (y, x)
// of the left site (none: every horizontal bond above the last row); the *_sc entries hand it over, the others leave it off
struct SCPairArgs {
  int on = 0, n_bonds = 0;
  const int32_t *bonds = nullptr;
  std::vector<std::pair<size_t, size_t>> selected(const char *who) const {
    if (n_bonds < 0 || (n_bonds > 0 && !bonds)) throw std::invalid_argument(std::string(who) + ": reference bonds missing");
    std::vector<std::pair<size_t, size_t>> out;
    for (int k = 0; k < n_bonds; ++k) {
      if (bonds[2 * k] < 0 || bonds[2 * k + 1] < 0) throw std::invalid_argument(std::string(who) + ": negative reference bond coordinate");
      out.emplace_back((size_t)bonds[2 * k], (size_t)bonds[2 * k + 1]);
    }
    return out;
  }
};
template <typename Fn>
auto with_fermion_measurement_model(const char *who, int model, const double *prm, int n_prm, Fn &&fn, const SCPairArgs &sc = {}) {
  if (model < 0 || model > 3 || n_prm < 0 || n_prm > 5 || (n_prm > 0 && !prm))
    throw std::invalid_argument(std::string(who) + ": model 0 (spinless), 1 (tj), 2 (tjnn) or 3 (hubbard), at most 5 parameters");
  if (sc.on && model != 1 && model != 2) throw std::invalid_argument(std::string(who) + ": SC_singlet_pair_corr is an observable of the t-J models");
  double p[5] = {0, 0, 0, 0, 0};
  std::copy(prm, prm + n_prm, p);
  auto with_sc = [&](auto &m) {
    if (sc.on) { m.SetEnableSingletPairCorrelation(true); m.SetSelectedRefBonds(sc.selected(who)); }
    return fn(m);
  };
  if (model == 0) { SquareSpinlessFermion m(p[0], p[2], p[1]); return fn(m); }
  if (model == 1) { SquaretJVModel m(p[0], p[4], p[1], p[2], p[3]); return with_sc(m); }
  if (model == 3) { SquareHubbardModel m(p[0], p[1], p[2]); return fn(m); }      // [t, U, mu]
  SquaretJNNModel m(p[0], p[1], p[2]);
  return with_sc(m);
}
struct KeyedValues {            // the output of the three entries below
  std::string keys;
  std::vector<double> vals;
  template <typename V> void push(const V &v) {
    vals.push_back(std::real(v));
    if constexpr (!std::is_arithmetic_v<V>) vals.push_back(std::imag(v));
  }
  void write(const char *who, char *keys_out, int keys_cap, double *values_out, long values_cap, long *values_len) const {
    if (!keys_out || !values_out || !values_len) throw std::invalid_argument(std::string(who) + ": null output buffer");
    if ((int)keys.size() + 1 > keys_cap || (long)vals.size() > values_cap) throw std::out_of_range(std::string(who) + ": output buffer too small");
    std::copy(keys.begin(), keys.end(), keys_out);
    keys_out[keys.size()] = 0;
    std::copy(vals.begin(), vals.end(), values_out);
    *values_len = (long)vals.size();
  }
};
// EvaluateObservables on a batch of configurations: per key [walker][len], then psi_mean [walker] and psi_rel_err [walker]
template <typename TenElemT>
void fermion_observables_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat, int n,
                              const int32_t *configs, int model, int n_prm, const double *prm, KeyedValues &out, const SCPairArgs &sc = {}) {
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor, &dec);
  with_fermion_measurement_model("pepshost_fermion_observables", model, prm, n_prm, [&](auto &m) {
    ObservableMapT<TenElemT> obs = m.EvaluateObservables(sitps, comp);
    for (const auto &kv : obs.values) {
      out.keys += kv.first + ":" + std::to_string(obs.len(kv.first)) + ";";
      for (const auto &v : kv.second) out.push(v);
    }
    const PsiSummaryT<TenElemT> psi = m.template EvaluatePsiSummaryT<TenElemT>();
    for (const auto &v : psi.psi_mean) out.push(v);
    for (double v : psi.psi_rel_err) out.push(TenElemT(v));
    return 0;
  }, sc);
}
// ExactSumMeasurer, the share of one rank: values = [weight | per key the raw weighted sums] (pepshost_exact_sum_measure_partial)
template <typename TenElemT>
void fermion_exact_sum_measure_partial_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat,
                                            const int32_t *all_configs, int n_configs, int model, int n_prm, const double *prm, int rank,
                                            int size, int batch, KeyedValues &out, const SCPairArgs &sc = {}) {
  if (n_configs < 1 || !all_configs || batch < 1 || size < 1 || rank < 0 || rank >= size)
    throw std::invalid_argument("pepshost_fermion_exact_sum_measure_partial: configurations, batch >= 1 and 0 <= rank < size are required");
  if (rank >= n_configs) { out.vals.assign(1, 0.0); return; }          // a rank without configurations contributes nothing
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  auto capture = [&](std::vector<double> &v) { out.vals = v; v[0] = 1.0; };   // keep the raw sums; normalise in the caller
  with_fermion_measurement_model("pepshost_fermion_exact_sum_measure_partial", model, prm, n_prm, [&](auto &m) {
    const auto res = ExactSumMeasurer(sitps, all, contractor, m, rank, size, (size_t)batch, capture, nullptr, &dec);
    for (const auto &kv : res) out.keys += kv.first + ":" + std::to_string(kv.second.size()) + ";";
    return 0;
  }, sc);
}
// MCPEPSMeasurer with the exchange updater: per key mean [len] and standard error [len] across the walkers, then the psi summary of the
// last sample.  Warm-up, samples and random streams as fermion_measure_energy_impl (no rescaling of the state), so energy_samples_out
// [sample][walker] holds the numbers that entry returns.
template <typename TenElemT>
void fermion_measure_impl(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat, int n,
                          int32_t *configs, const uint64_t *seeds, int warmup_sweeps, int n_samples, int sweeps_between, int model, int n_prm,
                          const double *prm, KeyedValues &out, double *energy_samples_out, double *accept_out, int updater = 0,
                          const SCPairArgs &sc = {}) {
  if (n_samples < 1 || warmup_sweeps < 0 || sweeps_between < 0 || !seeds || !configs)
    throw std::invalid_argument("pepshost_fermion_measure: seeds, configurations and n_samples >= 1 are required");
  if (updater != 0 && updater != 3) throw std::invalid_argument("pepshost_fermion_measure: updater must be 0 (exchange) or 3 (hubbard_u1u1)");
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), n, dtype, g_device);
  TPSWaveFunctionComponentT<TenElemT> comp(sitps, make_cfg(n, rows, cols, configs), contractor, &dec);
  std::vector<uint64_t> sd(seeds, seeds + n);
  MCUpdateSquareNNExchangeOBC ex(sd);
  MCUpdateSquareNNHubbardU1U1OBC hub(sd);
  MCMeasurementParams mp;
  mp.num_samples = n_samples; mp.num_warmup_sweeps = warmup_sweeps; mp.sweeps_between_samples = sweeps_between;
  mp.normalize_state = false;
  constexpr int z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  auto report = [&](auto &meas) {
    meas.Execute();
    for (const auto &kv : meas.ObservableRegistry()) {
      out.keys += kv.first + ":" + std::to_string(kv.second.first.size()) + ";";
      for (const auto &v : kv.second.first) out.push(v);
      for (size_t k = 0; k < kv.second.first.size(); ++k) out.push(TenElemT(kv.second.second.empty() ? 0.0 : kv.second.second[k]));
    }
    for (int w = 0; w < n; ++w) out.push(meas.PsiSamples().back()[w].first);
    for (int w = 0; w < n; ++w) out.push(TenElemT(meas.PsiSamples().back()[w].second));
    if (energy_samples_out)
      for (size_t k = 0; k < meas.EnergySamples().size(); ++k) copy_out(meas.EnergySamples()[k], energy_samples_out + k * (size_t)n * z);
    if (accept_out) std::copy(meas.AcceptRates().begin(), meas.AcceptRates().end(), accept_out);
  };
  with_fermion_measurement_model("pepshost_fermion_measure", model, prm, n_prm, [&](auto &m) {
    if (updater == 3) {
      MCPEPSMeasurer<MCUpdateSquareNNHubbardU1U1OBC, std::decay_t<decltype(m)>, TenElemT> meas(sitps, comp, mp, hub, m);
      report(meas);
    } else {
      MCPEPSMeasurer<MCUpdateSquareNNExchangeOBC, std::decay_t<decltype(m)>, TenElemT> meas(sitps, comp, mp, ex, m);
      report(meas);
    }
    return 0;
  }, sc);
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
}

// ---- the device-resident Optimizer on a fermionic state (sitps_ext_flat: the 4 d decorated components; bond_parity
// [rows][cols][4][D]).  model 0: SquareSpinlessFermion, prm = [t, V, t2, -]; model 1: SquaretJVModel, prm = [t, J, V, mu, (t2)].
// state_out: the d stored components (variant 0), [rows][cols][d][D^4]. ----
template <typename TenElemT, typename Fn>
auto with_fermion_model(int model, const double *prm, int n_prm, Fn &&fn) {
  if (model != 0 && model != 1 && model != 3) throw std::invalid_argument("fermionic optimizer: model must be 0 (spinless), 1 (tj) or 3 (hubbard)");
  if (!prm || n_prm < (model == 3 ? 3 : 4)) throw std::invalid_argument("fermionic optimizer: at least four model parameters (hubbard: three)");
  if (model == 0) { SquareSpinlessFermion m(prm[0], prm[2], prm[1]); return fn(m); }
  if (model == 3) { SquareHubbardModel m(prm[0], prm[1], prm[2]); return fn(m); }
  SquaretJVModel m(prm[0], n_prm > 4 ? prm[4] : 0.0, prm[1], prm[2], prm[3]);
  return fn(m);
}
inline FermionDecoration make_decoration(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity) {
  if (d < 1 || !nf || !bond_parity) throw std::invalid_argument("fermionic optimizer: d, nf and bond_parity are required");
  FermionDecoration dec;
  dec.nf.assign(nf, nf + d);
  dec.bond_parity.assign(bond_parity, bond_parity + (size_t)rows * cols * 4 * D);
  return dec;
}

template <typename TenElemT>
void fermion_optimize_exact_sum_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                     const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model, const double *prm,
                                     int n_prm, int rule, double lr, const double *rule_params, int n_rule_params, int iterations,
                                     double clip_value, double clip_norm, int batch, double *energies_out, double *grad_norms_out,
                                     double *state_out) {
  if (iterations < 0 || n_configs < 1 || batch < 1) throw std::invalid_argument("pepshost_fermion_optimize_exact_sum: bad iterations / n_configs / batch");
  static const int want[3] = {3, 2, 4};
  if (rule < 0 || rule > 2 || n_rule_params != want[rule] || !rule_params)
    throw std::invalid_argument("pepshost_fermion_optimize_exact_sum: rule 0 SGD (3 parameters), 1 AdaGrad (2), 2 Adam (4)");
  const FermionDecoration dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  OptimizerParams::BaseParams base((size_t)iterations, 0.0, 0.0, (size_t)iterations + 1, lr);   // the stopping criteria are off
  if (clip_value > 0.0) base.clip_value = clip_value;
  if (clip_norm > 0.0) base.clip_norm = clip_norm;
  const double *q = rule_params;
  AlgorithmParams algo = rule == 0   ? AlgorithmParams(SGDParams(q[0], q[1] != 0.0, q[2]))
                         : rule == 1 ? AlgorithmParams(AdaGradParams(q[0], q[1]))
                                     : AlgorithmParams(AdamParams(q[0], q[1], q[2], q[3]));
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(base, algo), contractor, &dec);
  typename Optimizer<TenElemT>::OptimizationResult res = with_fermion_model<TenElemT>(model, prm, n_prm, [&](auto &m) {
    return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) { return ExactSumAccumulateResident(sitps, all, c, m, (size_t)batch, &dec); });
  });
  copy_out(res.energy_trajectory, energies_out);
  if (grad_norms_out) std::copy(res.gradient_norms.begin(), res.gradient_norms.end(), grad_norms_out);
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
}

// ---- L-BFGS (LBFGSParams) with the exact-summation evaluator, the whole loop in one call.  lbfgs = the fourteen fields of LBFGSParams in
// their order (step_mode 0 fixed, 1 strong Wolfe; the two flags as 0 / 1).  energies_out / grad_norms_out: up to iterations + 1 entries,
// steps_out: up to iterations; info_out = [energies written, steps written, skipped pairs, damped pairs, descent resets, line-search
// evaluations, converged].  state_out is written on every exit, a failed line search included (the state is then the base of that search).
inline LBFGSParams make_lbfgs(const double *q) {
  if (!q) throw std::invalid_argument("L-BFGS: the parameter array is required");
  for (int i : {0, 3}) if (!(q[i] >= 0.0 && q[i] < 1e9)) throw std::invalid_argument("L-BFGS: history_size / max_eval out of range");
  return LBFGSParams((size_t)q[0], q[1], q[2], (size_t)q[3], q[4] != 0.0 ? LBFGSStepMode::kStrongWolfe : LBFGSStepMode::kFixed, q[5], q[6],
                     q[7], q[8], q[9], q[10] != 0.0, q[11], q[12] != 0.0, q[13]);
}
template <typename TenElemT, typename Run>
void lbfgs_drive(Optimizer<TenElemT> &opt, Run &&run, int rows, int cols, int d, int D, double *energies_out, double *grad_norms_out,
                 double *steps_out, double *state_out, double *info_out) {
  typename Optimizer<TenElemT>::OptimizationResult res;
  try {
    res = run();
  } catch (...) {
    copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
    throw;
  }
  copy_out(res.energy_trajectory, energies_out);
  if (grad_norms_out) std::copy(res.gradient_norms.begin(), res.gradient_norms.end(), grad_norms_out);
  if (steps_out) std::copy(res.learning_rate_trajectory.begin(), res.learning_rate_trajectory.end(), steps_out);
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
  if (info_out) {
    info_out[0] = (double)res.energy_trajectory.size(); info_out[1] = (double)res.learning_rate_trajectory.size();
    info_out[2] = (double)res.lbfgs_skip_curvature_count; info_out[3] = (double)res.lbfgs_damping_count;
    info_out[4] = (double)res.lbfgs_descent_reset_count; info_out[5] = (double)res.lbfgs_line_search_evaluations;
    info_out[6] = res.converged ? 1.0 : 0.0;
  }
}
inline OptimizerParams::BaseParams lbfgs_base(int iterations, double energy_tolerance, double gradient_tolerance, int plateau_patience,
                                              double lr) {
  // a patience <= 0 switches the plateau criterion off, as the tolerances of 0 do theirs
  return OptimizerParams::BaseParams((size_t)iterations, energy_tolerance, gradient_tolerance,
                                     plateau_patience > 0 ? (size_t)plateau_patience : (size_t)iterations + 1, lr);
}

template <typename TenElemT>
void lbfgs_exact_sum_impl(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, const int32_t *all_configs,
                          int n_configs, int model, const double *p, double lr, const double *lbfgs, int iterations,
                          double energy_tolerance, double gradient_tolerance, int plateau_patience, int batch, double *energies_out,
                          double *grad_norms_out, double *steps_out, double *state_out, double *info_out) {
  if (iterations < 0 || n_configs < 1 || batch < 1) throw std::invalid_argument("pepshost_lbfgs_exact_sum: bad iterations / n_configs / batch");
  if (model < 0 || model > 4) throw std::invalid_argument("pepshost_lbfgs_exact_sum: model must be xxz, tfim, j1j2, triangle or trij1j2");
  const LBFGSParams lp = make_lbfgs(lbfgs);
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(lbfgs_base(iterations, energy_tolerance, gradient_tolerance, plateau_patience, lr), lp), contractor);
  auto run = [&](auto &m) {
    return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) { return ExactSumAccumulateResident(sitps, all, c, m, (size_t)batch); });
  };
  lbfgs_drive(opt, [&]() {
    if (model == 0) { SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]); return run(m); }
    if (model == 2) { SquareSpinOneHalfJ1J2XXZModelOBC m(p[0], p[1], p[2], p[3], p[4]); return run(m); }
    if (model == 3) { SpinOneHalfTriHeisenbergSqrPEPS m; return run(m); }
    if (model == 4) { SpinOneHalfTriJ1J2HeisenbergSqrPEPS m(p[0]); return run(m); }
    TransverseFieldIsingSquareOBC m(p[0]);
    return run(m);
  }, rows, cols, d, D, energies_out, grad_norms_out, steps_out, state_out, info_out);
}

template <typename TenElemT>
void fermion_lbfgs_exact_sum_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                  const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model, const double *prm,
                                  int n_prm, double lr, const double *lbfgs, int iterations, double energy_tolerance,
                                  double gradient_tolerance, int plateau_patience, int batch, double *energies_out, double *grad_norms_out,
                                  double *steps_out, double *state_out, double *info_out) {
  if (iterations < 0 || n_configs < 1 || batch < 1) throw std::invalid_argument("pepshost_fermion_lbfgs_exact_sum: bad iterations / n_configs / batch");
  const LBFGSParams lp = make_lbfgs(lbfgs);
  const FermionDecoration dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(lbfgs_base(iterations, energy_tolerance, gradient_tolerance, plateau_patience, lr), lp), contractor,
                          &dec);
  lbfgs_drive(opt, [&]() {
    return with_fermion_model<TenElemT>(model, prm, n_prm, [&](auto &m) {
      return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) { return ExactSumAccumulateResident(sitps, all, c, m, (size_t)batch, &dec); });
    });
  }, rows, cols, d, D, energies_out, grad_norms_out, steps_out, state_out, info_out);
}

// sr_step_samples_impl on a fermionic state; info_out as there, the norms over the stored parameters
template <typename TenElemT>
void fermion_sr_step_samples_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                  const double *sitps_ext_flat, int n, const int32_t *configs, int model, const double *prm, int n_prm,
                                  double lr, double diag_shift, int cg_max_iter, double cg_relative_tolerance, int normalize_update,
                                  double *state_out, double *info_out) {
  if (n < 1 || cg_max_iter < 0) throw std::invalid_argument("pepshost_fermion_sr_step_samples: bad sample count / CG iterations");
  const FermionDecoration dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, 4 * d, sitps_ext_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, 4 * d, trunc_params(chi), n, dtype, g_device);
  const Configuration samples = make_cfg(n, rows, cols, configs);
  StochasticReconfigurationParams sr;
  sr.cg_params.max_iter = (size_t)cg_max_iter;
  sr.cg_params.relative_tolerance = cg_relative_tolerance;
  sr.diag_shift = diag_shift;
  sr.normalize_update = normalize_update != 0;
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(OptimizerParams(OptimizerParams::BaseParams(1, 0.0, 0.0, 2, lr), sr), contractor, &dec);
  typename Optimizer<TenElemT>::OptimizationResult res = with_fermion_model<TenElemT>(model, prm, n_prm, [&](auto &m) {
    return opt.IterativeOptimize([&](BMPSContractorT<TenElemT> &c) { return SampleSetAccumulateResident(sitps, samples, c, m, &dec); });
  });
  info_out[0] = std::real(res.energy_trajectory.at(0)); info_out[1] = std::real(res.energy_trajectory.at(1));
  info_out[2] = (double)res.sr_iterations; info_out[3] = res.sr_natural_grad_norm; info_out[4] = res.sr_residual_norm;
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
}

// ---- Monte-Carlo VMC on the resident state: MCEnergyGradEvaluator and VMCPEPSOptimizer (qlpeps_gpu.h) ----
// One description for the bosonic and the fermionic entries: nf == nullptr is a bosonic state ([rows][cols][d][D^4], models xxz 0, tfim 1,
// j1j2 2; updaters exchange 0, fullspace 1, tnn3 2); else sitps_flat holds the 4 d decorated components and bond_parity the bond parities
// (models spinless 0, tj 1, hubbard 3; updaters exchange 0, tnn3 2, hubbard_u1u1 3).
// algo: 0 SGD (momentum, nesterov, weight_decay), 1 AdaGrad (epsilon, initial_accumulator_value), 2 Adam (beta1, beta2, epsilon,
// weight_decay), 3 SR (diag_shift, cg_max_iter, cg_relative_tolerance, normalize_update), 4 MinSR (r_pinv, a_pinv, soft_cutoff),
// 5 L-BFGS (the fourteen fields of LBFGSParams).
struct VMCSpec {
  int warmup_sweeps = 0, samples_per_walker = 1, sweeps_between = 1;
  int algo = 0, n_rule_params = 0, iterations = 0;
  double lr = 0.0, clip_value = 0.0, clip_norm = 0.0;
  const double *rule_params = nullptr;
};
inline AlgorithmParams make_vmc_algo(const VMCSpec &v) {
  static const int want[6] = {3, 2, 4, 4, 3, 14};
  if (v.algo < 0 || v.algo > 5 || !v.rule_params || v.n_rule_params != want[v.algo])
    throw std::invalid_argument("vmc: algo 0 SGD (3 parameters), 1 AdaGrad (2), 2 Adam (4), 3 SR (4), 4 MinSR (3), 5 L-BFGS (14)");
  const double *q = v.rule_params;
  if (v.algo == 0) return SGDParams(q[0], q[1] != 0.0, q[2]);
  if (v.algo == 1) return AdaGradParams(q[0], q[1]);
  if (v.algo == 2) return AdamParams(q[0], q[1], q[2], q[3]);
  if (v.algo == 3) {
    if (!(q[1] >= 0.0 && q[1] < 1e9)) throw std::invalid_argument("vmc: SR cg_max_iter out of range");
    StochasticReconfigurationParams sr;
    sr.diag_shift = q[0]; sr.cg_params.max_iter = (size_t)q[1]; sr.cg_params.relative_tolerance = q[2]; sr.normalize_update = q[3] != 0.0;
    return sr;
  }
  if (v.algo == 4) return MinSRParams(q[0], q[1], q[2] != 0.0);
  return make_lbfgs(q);
}
inline VMCPEPSOptimizerParams make_vmc_params(const VMCSpec &v, int chi, const char *tps_base, const char *energy_dir, const char *config_dir) {
  if (v.iterations < 0 || v.warmup_sweeps < 0 || v.sweeps_between < 0 || v.samples_per_walker < 0)
    throw std::invalid_argument("vmc: negative iterations / sweeps / samples");
  OptimizerParams::BaseParams base((size_t)v.iterations, 0.0, 0.0, (size_t)v.iterations + 1, v.lr);   // the stopping criteria are off
  if (v.clip_value > 0.0) base.clip_value = v.clip_value;
  if (v.clip_norm > 0.0) base.clip_norm = v.clip_norm;
  MonteCarloParams mc;
  mc.num_warmup_sweeps = (size_t)v.warmup_sweeps; mc.sweeps_between_samples = (size_t)v.sweeps_between;
  mc.samples_per_walker = (size_t)v.samples_per_walker;
  mc.config_dump_path = config_dir ? config_dir : "";
  VMCPEPSOptimizerParams vp(OptimizerParams(base, make_vmc_algo(v)), mc, trunc_params(chi), tps_base ? tps_base : "");
  vp.energy_dump_dir = energy_dir ? energy_dir : "";
  return vp;
}
// (updater, model) of the ids -> fn(updater object, model object); dry: CheckModelUpdaterPair only, no object is built.  A pair that
// CheckModelUpdaterPair refuses is not instantiated.
template <class U, class M>
constexpr bool kVMCPairBuilt = !(std::is_same<U, MCUpdateSquareNNHubbardU1U1OBC>::value && !std::is_same<M, SquareHubbardModel>::value) &&
                               !(std::is_same<M, TransverseFieldIsingSquareOBC>::value && !std::is_same<U, MCUpdateSquareNNFullSpaceUpdateOBC>::value) &&
                               !(IsFermionicModel<M>::value && std::is_same<U, MCUpdateSquareNNFullSpaceUpdateOBC>::value);
template <class U, class M, typename Fn>
void vmc_pair(const std::vector<uint64_t> &sd, M &m, bool dry, Fn &&fn) {
  CheckModelUpdaterPair<U, M>(IsFermionicModel<M>::value);
  if constexpr (kVMCPairBuilt<U, M>) {
    if (dry) return;
    U u(sd);
    fn(u, m);
  }
}
template <typename Fn>
void with_vmc_pair(bool fermion, int updater, int model, const double *p, int n_prm, const std::vector<uint64_t> &sd, bool dry, Fn &&fn) {
  auto on_model = [&](auto &m) {
    using M = std::decay_t<decltype(m)>;
    if (updater == 0) vmc_pair<MCUpdateSquareNNExchangeOBC, M>(sd, m, dry, fn);
    else if (updater == 1) vmc_pair<MCUpdateSquareNNFullSpaceUpdateOBC, M>(sd, m, dry, fn);
    else if (updater == 2) vmc_pair<MCUpdateSquareTNN3SiteExchange, M>(sd, m, dry, fn);
    else if (updater == 3) vmc_pair<MCUpdateSquareNNHubbardU1U1OBC, M>(sd, m, dry, fn);
    else throw std::invalid_argument("vmc: updater must be 0 (exchange), 1 (fullspace), 2 (tnn3) or 3 (hubbard_u1u1)");
    return 0;
  };
  if (!p) throw std::invalid_argument("vmc: the model parameters are required");
  if (fermion) { with_fermion_model<double>(model, p, n_prm, on_model); return; }
  if (model == 0) { SquareSpinOneHalfXXZModelOBC m(p[0], p[1], p[2]); on_model(m); }
  else if (model == 1) { TransverseFieldIsingSquareOBC m(p[0]); on_model(m); }
  else if (model == 2) { SquareSpinOneHalfJ1J2XXZModelOBC m(p[0], p[1], p[2], p[3], p[4]); on_model(m); }
  else throw std::invalid_argument("vmc: a bosonic model must be 0 (xxz), 1 (tfim) or 2 (j1j2)");
}
// the d stored components of an extended state (variant 0), or the state itself
template <typename TenElemT>
void copy_stored_out(const SplitIndexTPST<TenElemT> &ext, size_t d_stored, double *out) {
  if (!out) return;
  constexpr size_t z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  for (size_t r = 0; r < ext.rows(); ++r)
    for (size_t c = 0; c < ext.cols(); ++c)
      for (size_t k = 0; k < d_stored; ++k) {
        const double *src = dptr(ext.component(r, c, k));
        std::copy(src, src + z * ext.slot(), out + z * (((r * ext.cols() + c) * d_stored + k) * ext.slot()));
      }
}

// VMCPEPSOptimizer::Execute in one call.  Outputs ([iterations + 1] = one entry per evaluation): energies (re [, im]), their binned
// errors, gradient norms, accept [evaluation][walker]; state_out / lowest_out: the d stored components of GetState / GetLowestState;
// info_out (7 doubles) = [evaluations, GetMinEnergy, max_w |psi_w| of the walkers at return, GetCurrentEnergy (re), seconds in the
// evaluator, in IterativeOptimize, in all (GetTimings)]; configs: the final configurations.  finalize == 0 stops before the closing RefreshWavefunctionComponent + NormalizeStateOrder1 (theta as the last step
// left it).  probe_iteration >= 0: an OptimizationCallback reads GetState() into probe_state_out at that iteration.
template <typename TenElemT>
void vmc_optimize_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                       const double *sitps_flat, int n, int32_t *configs, const uint64_t *seeds, int n_seeds, int updater, int model,
                       const double *p, int n_prm, const VMCSpec &spec, int finalize, int probe_iteration, const char *tps_base,
                       const char *energy_dir, const char *config_dir, double *energies_out, double *errors_out, double *grad_norms_out,
                       double *accept_out, double *state_out, double *lowest_out, double *probe_state_out, double *info_out) {
  // every refusal that needs no device comes first
  if (n < 0 || n_seeds < 0 || (n > 0 && !configs) || (n_seeds > 0 && !seeds) || !sitps_flat) throw std::invalid_argument("vmc: null / negative argument");
  const VMCPEPSOptimizerParams vp = make_vmc_params(spec, chi, tps_base, energy_dir, config_dir);
  vp.Validate((size_t)n, (size_t)n_seeds);
  const bool fermion = nf != nullptr;
  const std::vector<uint64_t> sd(seeds, seeds + n_seeds);
  with_vmc_pair(fermion, updater, model, p, n_prm, sd, /*dry=*/true, [](auto &, auto &) {});
  FermionDecoration dec;
  if (fermion) dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  const int dev_d = fermion ? 4 * d : d;
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, dev_d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, dev_d, vp.peps_params, n, dtype, g_device);
  contractor.UploadState(sitps);
  TPSWaveFunctionComponentT<TenElemT> comp(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), make_cfg(n, rows, cols, configs),
                                           contractor, fermion ? &dec : nullptr);
  with_vmc_pair(fermion, updater, model, p, n_prm, sd, /*dry=*/false, [&](auto &upd, auto &m) {
    VMCPEPSOptimizer<std::decay_t<decltype(upd)>, std::decay_t<decltype(m)>, TenElemT> exe(vp, comp, upd, m, sd.size(), (size_t)D);
    if (probe_iteration >= 0 && probe_state_out) {
      typename Optimizer<TenElemT>::OptimizationCallback cb;
      cb.on_iteration = [&](size_t it, double, double, double) {
        if ((long)it == (long)probe_iteration) copy_out(exe.GetState().flat(), probe_state_out);
      };
      exe.SetOptimizationCallback(cb);
    }
    if (finalize) exe.Execute();
    else { exe.WarmUpAndOptimize(); exe.DumpData(); }
    copy_out(exe.GetEnergyTrajectory(), energies_out);
    const size_t ne = exe.GetEnergyTrajectory().size();
    if (errors_out) std::copy(exe.GetEnergyErrorTrajectory().begin(), exe.GetEnergyErrorTrajectory().end(), errors_out);
    if (grad_norms_out) std::copy(exe.GetGradientNormTrajectory().begin(), exe.GetGradientNormTrajectory().end(), grad_norms_out);
    if (accept_out)
      for (size_t k = 0; k < ne; ++k) {
        const auto &a = exe.GetAcceptRatesTrajectory()[k];
        for (size_t w = 0; w < (size_t)n; ++w) accept_out[k * n + w] = w < a.size() ? a[w] : 0.0;
      }
    copy_out(exe.GetState().flat(), state_out);
    copy_out(exe.GetLowestState().flat(), lowest_out);
    if (info_out) {
      double mx = 0.0;
      for (const auto &a : comp.amplitude) mx = std::max(mx, (double)std::abs(a));
      info_out[0] = (double)ne; info_out[1] = exe.GetMinEnergy(); info_out[2] = mx; info_out[3] = std::real(exe.GetCurrentEnergy());
      info_out[4] = exe.GetTimings().evaluation_s; info_out[5] = exe.GetTimings().optimize_s; info_out[6] = exe.GetTimings().total_s;
    }
  });
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
}

// MCEnergyGradEvaluator::Evaluate alone, n_evaluates times on one engine with no step between them (the chains persist), for tests.
// Warm-up: normalize != 0 is MonteCarloEngine::WarmUp (sweeps + NormalizeStateOrder1 on the device), else the plain sweeps.  Per
// evaluation k: energy_samples_out [k][sample][walker], so_out / seo_out [k][state size] (pepsgpu_grad_read), scalars_out [k][5] =
// (e_loc_sum re, im, weight_sum, energy_error, samples in the SR store), accept_out [k][walker].  spec.algo >= 0 with state_out: after the
// last evaluation the step is composed by hand on the contractor -- finish, clip (first-order rules), [natural gradient | MinSR
// direction], step -- and theta is read back (the d stored components); step_info_out = [energy re, gradient norm].
template <typename TenElemT>
void mc_evaluate_resident_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                               const double *sitps_flat, int n, int32_t *configs, const uint64_t *seeds, int updater, int model,
                               const double *p, int n_prm, int warmup_sweeps, int normalize, int n_samples, int n_evaluates, int collect_sr,
                               const VMCSpec &spec, double *energy_samples_out, double *so_out, double *seo_out, double *scalars_out,
                               double *accept_out, double *state_out, double *step_info_out) {
  if (n < 1 || !configs || !seeds || !sitps_flat || n_samples < 1 || n_evaluates < 1 || warmup_sweeps < 0)
    throw std::invalid_argument("pepshost_mc_evaluate_resident: walkers, seeds, n_samples >= 1 and n_evaluates >= 1 are required");
  const bool fermion = nf != nullptr, step = spec.algo >= 0 && state_out;
  const std::vector<uint64_t> sd(seeds, seeds + n);
  with_vmc_pair(fermion, updater, model, p, n_prm, sd, /*dry=*/true, [](auto &, auto &) {});
  AlgorithmParams algo = SGDParams();
  if (step) algo = make_vmc_algo(spec);
  if (step && spec.algo == 5) throw std::invalid_argument("pepshost_mc_evaluate_resident: the hand-composed step covers SGD, AdaGrad, Adam, SR and MinSR");
  FermionDecoration dec;
  if (fermion) dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  const int dev_d = fermion ? 4 * d : d;
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, dev_d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, dev_d, trunc_params(chi), n, dtype, g_device);
  contractor.UploadState(sitps);
  TPSWaveFunctionComponentT<TenElemT> comp(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), make_cfg(n, rows, cols, configs),
                                           contractor, fermion ? &dec : nullptr);
  // (the Optimizer object is only the RAII holder of pepsgpu_opt_begin / _end and of the decoration; no method of it steps here)
  Optimizer<TenElemT> opt(OptimizerParams(OptimizerParams::BaseParams(0, 0.0, 0.0, 1, 0.0), algo), contractor, fermion ? &dec : nullptr);
  MonteCarloParams mc;
  mc.num_warmup_sweeps = (size_t)warmup_sweeps; mc.samples_per_walker = (size_t)n_samples;
  constexpr size_t z = ElemTraits<TenElemT>::is_complex ? 2 : 1;
  with_vmc_pair(fermion, updater, model, p, n_prm, sd, /*dry=*/false, [&](auto &upd, auto &m) {
    using U = std::decay_t<decltype(upd)>;
    using M = std::decay_t<decltype(m)>;
    MonteCarloEngine<U, TenElemT> engine(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), sitps, comp, mc, upd);
    if (normalize) engine.WarmUp();
    else for (int s = 0; s < warmup_sweeps; ++s) (void)engine.StepSweep(1);
    MCEnergyGradEvaluator<U, M, TenElemT> evaluator(engine, m, mc, collect_sr != 0 || (step && (spec.algo == 3 || spec.algo == 4)),
                                                    fermion ? &dec : nullptr);
    const size_t ns = (size_t)n * n_samples, sz = sitps.flat().size();
    DeviceEvaluationT<TenElemT> ev;
    for (int k = 0; k < n_evaluates; ++k) {
      ev = evaluator.Evaluate(contractor);
      if (energy_samples_out) copy_out(ev.energy_samples, energy_samples_out + z * ns * k);
      if (so_out && seo_out) {
        std::vector<TenElemT> so, seo;
        contractor.GradRead(so, seo);
        copy_out(so, so_out + z * sz * k);
        copy_out(seo, seo_out + z * sz * k);
      }
      if (scalars_out) {
        double *sc = scalars_out + 5 * k;
        sc[0] = std::real(ev.e_loc_sum); sc[1] = std::imag(ev.e_loc_sum); sc[2] = ev.weight_sum; sc[3] = ev.energy_error;
        sc[4] = (double)contractor.SRCount();
      }
      if (accept_out) std::copy(ev.accept_rates_avg.begin(), ev.accept_rates_avg.end(), accept_out + (size_t)n * k);
    }
    if (step) {
      const auto eg = contractor.OptGradientFromAccumulators(ev.e_loc_sum, ev.weight_sum);
      const double *q = spec.rule_params;
      if (spec.algo <= 2 && (spec.clip_value > 0.0 || spec.clip_norm > 0.0)) contractor.OptClip(spec.clip_value, spec.clip_norm);
      if (spec.algo == 0) contractor.OptStep(0, spec.lr, {q[0], q[1] != 0.0 ? 1.0 : 0.0, q[2]});
      else if (spec.algo == 1) contractor.OptStep(1, spec.lr, {q[0], q[1]});
      else if (spec.algo == 2) contractor.OptStep(2, spec.lr, {q[0], q[1], q[2], q[3]});
      else if (spec.algo == 3) {
        const ConjugateGradientParams cg;
        const auto info = contractor.OptNaturalGradient(q[0], (size_t)q[1], q[2], cg.absolute_tolerance, cg.residual_recompute_interval,
                                                        cg.orthogonality_threshold);
        contractor.OptStep(0, q[3] != 0.0 && info.direction_norm > 0.0 ? spec.lr / info.direction_norm : spec.lr, {0.0, 0.0, 0.0});
      } else {
        contractor.MinSRDirection(ev.energy_samples, eg.first, q[0], q[1], q[2] != 0.0);
        contractor.OptStep(0, spec.lr, {0.0, 0.0, 0.0});
      }
      SplitIndexTPST<TenElemT> theta(rows, cols, dev_d, D);
      contractor.OptReadState(theta);
      copy_stored_out(theta, (size_t)d, state_out);
      if (step_info_out) { step_info_out[0] = std::real(eg.first); step_info_out[1] = eg.second; }
    }
  });
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
}

// ---- spike recovery, step selectors and checkpoints around the Optimizer (qlpeps_gpu.h: SpikeGuard, OptimizerParams) ----
// guard = 24 doubles: [0] enable_auto_recover, [1] redo_mc_max_retries, [2] factor_err, [3] factor_grad, [4] factor_ngrad,
// [5] sr_min_iters_suspicious, [6] enable_rollback, [7] ema_window, [8] sigma_k; [9] initial selector enabled, [10] max_line_search_steps,
// [11] enable_in_deterministic; [12] periodic selector enabled, [13] every_n_steps, [14] phase_switch_ratio, [15] enable_in_deterministic;
// [16] checkpoint every_n_steps; [17] lr_scheduler (0 none, 1 ConstantLR at lr); [18] energy_tolerance, [19] gradient_tolerance,
// [20] plateau_patience (<= 0: off); [21] probe_iteration (< 0: none); [22] capacity of events_out in events; [23] unused.
// The OptimizerParams are built with the four-argument constructor: enable_auto_recover is what [0] says.
struct GuardSpec {
  const double *g = nullptr;
  const char *csv_path = nullptr, *checkpoint_path = nullptr;
  const double *error_override = nullptr, *energy_shift = nullptr;   // the schedule, one entry per evaluator call
  int n_schedule = 0;                                                // 0: no schedule, the evaluator is not wrapped
};
inline size_t guard_count(double x, const char *what) {
  if (!(x >= 0.0 && x < 1e9)) throw std::invalid_argument(std::string("guard: ") + what + " out of range");
  return (size_t)x;
}
inline SpikeRecoveryParams make_spike_params(const double *g, const char *csv_path) {
  if (!g) throw std::invalid_argument("guard: the parameter array is required");
  SpikeRecoveryParams sp;
  sp.enable_auto_recover = g[0] != 0.0; sp.redo_mc_max_retries = guard_count(g[1], "redo_mc_max_retries");
  sp.factor_err = g[2]; sp.factor_grad = g[3]; sp.factor_ngrad = g[4];
  sp.sr_min_iters_suspicious = guard_count(g[5], "sr_min_iters_suspicious");
  sp.enable_rollback = g[6] != 0.0; sp.ema_window = guard_count(g[7], "ema_window"); sp.sigma_k = g[8];
  sp.log_trigger_csv_path = csv_path ? csv_path : "";
  return sp;
}
inline OptimizerParams make_guarded_params(const GuardSpec &gs, int iterations, double lr, double clip_value, double clip_norm,
                                           const AlgorithmParams &algo) {
  const double *g = gs.g;
  const SpikeRecoveryParams sp = make_spike_params(g, gs.csv_path);
  if (iterations < 0) throw std::invalid_argument("guard: negative iterations");
  std::unique_ptr<LearningRateScheduler> sched;
  if (g[17] != 0.0) sched = std::make_unique<ConstantLR>(lr);
  OptimizerParams::BaseParams base((size_t)iterations, g[18], g[19], g[20] > 0.0 ? guard_count(g[20], "plateau_patience") : (size_t)iterations + 1, lr,
                                   std::move(sched));
  if (clip_value > 0.0) base.clip_value = clip_value;
  if (clip_norm > 0.0) base.clip_norm = clip_norm;
  base.initial_step_selector.enabled = g[9] != 0.0;
  base.initial_step_selector.max_line_search_steps = guard_count(g[10], "max_line_search_steps");
  base.initial_step_selector.enable_in_deterministic = g[11] != 0.0;
  base.periodic_step_selector.enabled = g[12] != 0.0;
  base.periodic_step_selector.every_n_steps = guard_count(g[13], "every_n_steps");
  base.periodic_step_selector.phase_switch_ratio = g[14];
  base.periodic_step_selector.enable_in_deterministic = g[15] != 0.0;
  CheckpointParams ck;
  ck.every_n_steps = guard_count(g[16], "checkpoint every_n_steps");
  ck.base_path = gs.checkpoint_path ? gs.checkpoint_path : "";
  return OptimizerParams(base, algo, ck, sp);
}
// The schedule around an evaluator: at its k-th call error_override[k] (unless NaN) replaces the error bar and energy_shift[k] *
// weight_sum is added to e_loc_sum, which moves the energy and, through the finish, the gradient.  One call more than the schedule is
// long throws, so that no scripted run can loop.
template <typename TenElemT>
typename Optimizer<TenElemT>::Evaluator wrap_schedule(typename Optimizer<TenElemT>::Evaluator inner, const GuardSpec &gs,
                                                      std::shared_ptr<size_t> calls) {
  if (gs.n_schedule <= 0) return inner;
  return [inner, gs, calls](BMPSContractorT<TenElemT> &c) {
    const size_t k = (*calls)++;
    if (k >= (size_t)gs.n_schedule)
      throw std::runtime_error("guard: evaluator call " + std::to_string(k) + " is beyond the schedule of " + std::to_string(gs.n_schedule));
    DeviceEvaluationT<TenElemT> ev = inner(c);
    if (gs.error_override && !std::isnan(gs.error_override[k])) ev.energy_error = gs.error_override[k];
    if (gs.energy_shift) ev.e_loc_sum += TenElemT(gs.energy_shift[k] * ev.weight_sum);
    return ev;
  };
}
inline void write_events(const SpikeStatistics &st, size_t cap, double *events_out, double *counts_out) {
  const size_t n = std::min(cap, st.event_log.size());
  if (events_out)
    for (size_t i = 0; i < n; ++i) {
      const auto &e = st.event_log[i];
      double *o = events_out + 6 * i;
      o[0] = (double)e.step; o[1] = (double)e.attempt; o[2] = (double)(int)e.signal; o[3] = (double)(int)e.action; o[4] = e.value; o[5] = e.threshold;
    }
  if (counts_out) {
    counts_out[0] = (double)st.event_log.size(); counts_out[1] = (double)st.total_resamples; counts_out[2] = (double)st.total_rollbacks;
    counts_out[3] = (double)st.total_forced_accepts;
  }
}
// info_out (16 doubles) = [accepted evaluations, events, resamples, rollbacks, forced accepts, evaluator calls, energy-only calls,
// total_iterations, converged, min_energy, sr_iterations, sr_natural_grad_norm, sr_residual_norm, entries of selected_eta, lowest valid, -]
template <typename TenElemT>
void write_guarded_result(const typename Optimizer<TenElemT>::OptimizationResult &res, const GuardSpec &gs, double *energies_out,
                          double *errors_out, double *grad_norms_out, double *selected_eta_out, double *events_out, double *info_out) {
  copy_out(res.energy_trajectory, energies_out);
  if (errors_out) std::copy(res.energy_error_trajectory.begin(), res.energy_error_trajectory.end(), errors_out);
  if (grad_norms_out) std::copy(res.gradient_norms.begin(), res.gradient_norms.end(), grad_norms_out);
  if (selected_eta_out) std::copy(res.selected_eta.begin(), res.selected_eta.end(), selected_eta_out);
  if (info_out) {
    info_out[0] = (double)res.energy_trajectory.size();
    write_events(res.spike_stats, guard_count(gs.g[22], "events capacity"), events_out, info_out + 1);
    info_out[5] = (double)res.evaluator_calls; info_out[6] = (double)res.energy_only_calls; info_out[7] = (double)res.total_iterations;
    info_out[8] = res.converged ? 1.0 : 0.0; info_out[9] = res.min_energy; info_out[10] = (double)res.sr_iterations;
    info_out[11] = res.sr_natural_grad_norm; info_out[12] = res.sr_residual_norm; info_out[13] = (double)res.selected_eta.size();
  }
}

// Optimizer::IterativeOptimize with spike recovery, step selectors and checkpoints, on a fixed set of configurations.  algo as
// make_vmc_algo.  First-order rules and L-BFGS evaluate by exact summation over all_configs (optimize_exact_sum_impl); SR and MinSR
// need the sample store, so they take all_configs as a sample set of weight 1 (sr_step_samples_impl).  nf != NULL: a fermionic state
// (fermion_optimize_exact_sum_impl).  state_out is written on every exit, a throw from the loop included; lowest_out: theta at the
// lowest accepted energy (pepsgpu_vmc_snapshot_save); probe_state_out: theta when on_iteration reports iteration guard[21].
template <typename TenElemT>
void guarded_optimize_exact_sum_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                     const double *sitps_flat, const int32_t *all_configs, int n_configs, int model, const double *prm,
                                     int n_prm, const VMCSpec &spec, int batch, const GuardSpec &gs, double *energies_out, double *errors_out,
                                     double *grad_norms_out, double *selected_eta_out, double *events_out, double *state_out,
                                     double *lowest_out, double *probe_state_out, double *info_out) {
  // every refusal that needs no device comes first
  if (n_configs < 1 || batch < 1 || !all_configs || !sitps_flat || !prm) throw std::invalid_argument("pepshost_guarded_optimize_exact_sum: bad arguments");
  const OptimizerParams op = make_guarded_params(gs, spec.iterations, spec.lr, spec.clip_value, spec.clip_norm, make_vmc_algo(spec));
  op.ValidateGuards();
  const bool fermion = nf != nullptr, sample_set = spec.algo == 3 || spec.algo == 4;
  if (!fermion && (model < 0 || model > 4)) throw std::invalid_argument("pepshost_guarded_optimize_exact_sum: model must be xxz, tfim, j1j2, triangle or trij1j2");
  FermionDecoration dec;
  if (fermion) dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  const FermionDecoration *decp = fermion ? &dec : nullptr;
  const int dev_d = fermion ? 4 * d : d;
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, dev_d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, dev_d, trunc_params(chi), sample_set ? n_configs : batch, dtype, g_device);
  std::vector<std::vector<int32_t>> all(n_configs);
  for (int i = 0; i < n_configs; ++i) all[i].assign(all_configs + (size_t)i * rows * cols, all_configs + (size_t)(i + 1) * rows * cols);
  const Configuration samples = make_cfg(n_configs, rows, cols, all_configs);
  contractor.UploadState(sitps);
  Optimizer<TenElemT> opt(op, contractor, decp);
  auto calls = std::make_shared<size_t>(0);
  double lowest = std::numeric_limits<double>::max();
  bool has_lowest = false;
  typename Optimizer<TenElemT>::OptimizationCallback cb;
  cb.on_evaluation_accepted = [&](const DeviceEvaluationT<TenElemT> &, const TenElemT &e, size_t) {
    if (std::real(e) < lowest) { lowest = std::real(e); contractor.VMCSnapshotSave(); has_lowest = true; }
  };
  const long probe = (long)gs.g[21];
  if (probe >= 0 && probe_state_out)
    cb.on_iteration = [&](size_t it, double, double, double) {
      if ((long)it == probe) copy_out(opt.GetState(rows, cols, d, D).flat(), probe_state_out);
    };
  auto run = [&](auto &m) {
    typename Optimizer<TenElemT>::Evaluator inner = [&](BMPSContractorT<TenElemT> &c) {
      return sample_set ? SampleSetAccumulateResident(sitps, samples, c, m, decp) : ExactSumAccumulateResident(sitps, all, c, m, (size_t)batch, decp);
    };
    return opt.IterativeOptimize(wrap_schedule<TenElemT>(inner, gs, calls), cb);
  };
  typename Optimizer<TenElemT>::OptimizationResult res;
  try {
    if (fermion) res = with_fermion_model<TenElemT>(model, prm, n_prm, run);
    else if (model == 0) { SquareSpinOneHalfXXZModelOBC m(prm[0], prm[1], prm[2]); res = run(m); }
    else if (model == 2) { SquareSpinOneHalfJ1J2XXZModelOBC m(prm[0], prm[1], prm[2], prm[3], prm[4]); res = run(m); }
    else if (model == 3) { SpinOneHalfTriHeisenbergSqrPEPS m; res = run(m); }
    else if (model == 4) { SpinOneHalfTriJ1J2HeisenbergSqrPEPS m(prm[0]); res = run(m); }
    else { TransverseFieldIsingSquareOBC m(prm[0]); res = run(m); }
  } catch (...) {
    copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
    if (info_out) info_out[5] = (double)*calls;
    throw;
  }
  write_guarded_result<TenElemT>(res, gs, energies_out, errors_out, grad_norms_out, selected_eta_out, events_out, info_out);
  copy_out(opt.GetState(rows, cols, d, D).flat(), state_out);
  if (has_lowest && lowest_out) {
    SplitIndexTPST<TenElemT> snap(rows, cols, dev_d, D);
    contractor.VMCSnapshotRead(snap);
    copy_stored_out(snap, (size_t)d, lowest_out);
  }
  if (info_out) info_out[14] = has_lowest ? 1.0 : 0.0;
}

// vmc_optimize_impl with spike recovery, step selectors and checkpoints; the schedule wraps the executor's own evaluator
// (SetEnergyEvaluator).  No closing normalisation, no dumps.  accept_out [accepted evaluation][walker].
template <typename TenElemT>
void guarded_vmc_optimize_impl(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                               const double *sitps_flat, int n, int32_t *configs, const uint64_t *seeds, int n_seeds, int updater, int model,
                               const double *p, int n_prm, const VMCSpec &spec, const GuardSpec &gs, double *energies_out, double *errors_out,
                               double *grad_norms_out, double *selected_eta_out, double *events_out, double *accept_out, double *state_out,
                               double *lowest_out, double *info_out) {
  if (n < 0 || n_seeds < 0 || (n > 0 && !configs) || (n_seeds > 0 && !seeds) || !sitps_flat) throw std::invalid_argument("vmc: null / negative argument");
  VMCPEPSOptimizerParams vp = make_vmc_params(spec, chi, "", "", "");
  vp.optimizer_params = make_guarded_params(gs, spec.iterations, spec.lr, spec.clip_value, spec.clip_norm, make_vmc_algo(spec));
  vp.Validate((size_t)n, (size_t)n_seeds);
  const bool fermion = nf != nullptr;
  const std::vector<uint64_t> sd(seeds, seeds + n_seeds);
  with_vmc_pair(fermion, updater, model, p, n_prm, sd, /*dry=*/true, [](auto &, auto &) {});
  FermionDecoration dec;
  if (fermion) dec = make_decoration(rows, cols, D, d, nf, bond_parity);
  const int dev_d = fermion ? 4 * d : d;
  SplitIndexTPST<TenElemT> sitps = make_state_t<TenElemT>(rows, cols, D, dev_d, sitps_flat);
  BMPSContractorT<TenElemT> contractor(rows, cols, D, dev_d, vp.peps_params, n, dtype, g_device);
  contractor.UploadState(sitps);
  TPSWaveFunctionComponentT<TenElemT> comp(typename TPSWaveFunctionComponentT<TenElemT>::ResidentState(), make_cfg(n, rows, cols, configs),
                                           contractor, fermion ? &dec : nullptr);
  auto calls = std::make_shared<size_t>(0);
  with_vmc_pair(fermion, updater, model, p, n_prm, sd, /*dry=*/false, [&](auto &upd, auto &m) {
    VMCPEPSOptimizer<std::decay_t<decltype(upd)>, std::decay_t<decltype(m)>, TenElemT> exe(vp, comp, upd, m, sd.size(), (size_t)D);
    if (gs.n_schedule > 0) {
      exe.SetEnergyEvaluator(wrap_schedule<TenElemT>([&exe](BMPSContractorT<TenElemT> &c) { return exe.GetEvaluator().Evaluate(c); }, gs, calls));
      exe.SetEnergyOnlyEvaluator([&exe](BMPSContractorT<TenElemT> &c) { return exe.GetEvaluator().EvaluateEnergyOnly(c); });
    }
    const auto res = exe.WarmUpAndOptimize();
    write_guarded_result<TenElemT>(res, gs, nullptr, nullptr, grad_norms_out, selected_eta_out, events_out, info_out);
    copy_out(exe.GetEnergyTrajectory(), energies_out);           // the executor's own bookkeeping: accepted evaluations only
    const size_t ne = exe.GetEnergyTrajectory().size();
    if (errors_out) std::copy(exe.GetEnergyErrorTrajectory().begin(), exe.GetEnergyErrorTrajectory().end(), errors_out);
    if (accept_out)
      for (size_t k = 0; k < ne; ++k) {
        const auto &a = exe.GetAcceptRatesTrajectory()[k];
        for (size_t w = 0; w < (size_t)n; ++w) accept_out[k * n + w] = w < a.size() ? a[w] : 0.0;
      }
    copy_out(exe.GetState().flat(), state_out);
    copy_out(exe.GetLowestState().flat(), lowest_out);
    if (info_out) {
      info_out[0] = (double)ne; info_out[9] = exe.GetMinEnergy(); info_out[14] = 1.0;
      write_events(exe.GetSpikeStatistics(), guard_count(gs.g[22], "events capacity"), nullptr, info_out + 1);
    }
  });
  std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
}
}  // namespace

extern "C" {

const char *pepshost_last_error(void) { return g_err.c_str(); }

// HIP device of every contractor the calls below build (default: LOCAL_RANK of the launcher, else 0)
int pepshost_set_device(int device) {
  return guarded([&]() {
    if (device < 0) throw std::invalid_argument("pepshost_set_device: negative device index");
    g_device = device;
  });
}
int pepshost_get_device(void) { return g_device; }

// d_min < 0: D_min = chi.  scheme: 0 SVD_COMPRESS, 1 VARIATION2Site, 2 VARIATION1Site (bmps.h:31-35)
int pepshost_set_truncate_params(int d_min, double trunc_err, int scheme, double convergence_tol, int iter_max) {
  return guarded([&]() {
    if (scheme < 0 || scheme > 2) throw std::invalid_argument("unknown CompressMPSScheme");
    g_trunc.d_min = d_min; g_trunc.trunc_err = trunc_err; g_trunc.scheme = scheme; g_trunc.tol = convergence_tol; g_trunc.iters = iter_max;
  });
}

// n_sweeps Monte-Carlo sweeps (square_nn_updater.h:30-81) of n walkers; updater 0 = NN exchange,
// 1 = NN full-space (Suwa-Todo), 2 = three-site exchange (square_3site_updater.h:28-158).  configs are updated in place; one std::mt19937(seed[w]) per walker.
int pepshost_mc_sweeps(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n,
                       int32_t *configs, const uint64_t *seeds, int updater, int n_sweeps, double *amplitudes_out,
                       double *accept_rates_out) {
  return guarded([&]() {
    mc_sweeps_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, seeds, updater, n_sweeps, amplitudes_out, accept_rates_out);
  });
}
int pepshost_mc_sweeps_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n,
                            int32_t *configs, const uint64_t *seeds, int updater, int n_sweeps, double *amplitudes_out,
                            double *accept_rates_out) {
  return guarded([&]() {
    mc_sweeps_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, n, configs, seeds, updater, n_sweeps, amplitudes_out,
                                  accept_rates_out);
  });
}

// MonteCarloEngine (monte_carlo_engine.h:146-240, :340-414) on a walker batch: construction (configuration validity +
// rescue with the given amplitude window), WarmUp (warm-up sweeps with the NN exchange updater, sanity check,
// NormalizeStateOrder1).  In place: configs, sitps_flat (the scaled state).  out[0] = overall scale factor, out[1] = walkers
// rescued, out[2] = warmed up (0 / 1).
static int mc_engine_warmup_impl(int rows, int cols, int D, int d, int chi, int dtype, double *sitps_flat, int n, int32_t *configs,
                                 const uint64_t *seeds, int warmup_sweeps, int rescue_enabled, double amp_min, double amp_max,
                                 double *amplitudes_out, double *out, double (*max_over_ranks)(double),
                                 int (*exchange_valid_config)(int, int, int32_t *)) {
  return guarded([&]() {
    SplitIndexTPS sitps = make_state_t<double>(rows, cols, D, d, sitps_flat);
    BMPSContractor contractor(rows, cols, D, d, trunc_params(chi), n, dtype, g_device);
    TPSWaveFunctionComponent comp(sitps, make_cfg(n, rows, cols, configs), contractor);
    std::vector<uint64_t> sd(seeds, seeds + n);
    MCUpdateSquareNNExchangeOBC upd(sd);
    MonteCarloParams mp;
    mp.num_warmup_sweeps = (size_t)warmup_sweeps;
    ConfigurationRescueParams rp;
    rp.enabled = rescue_enabled != 0;
    if (amp_min > 0.0) rp.amplitude_min_threshold = amp_min;
    if (amp_max > 0.0) rp.amplitude_max_threshold = amp_max;
    std::function<double(double)> mx;
    std::function<int(int, int, int32_t *)> ex;
    if (max_over_ranks) mx = max_over_ranks;
    if (exchange_valid_config) ex = exchange_valid_config;
    MonteCarloEngine<MCUpdateSquareNNExchangeOBC> eng(sitps, comp, mp, upd, rp, mx, ex);
    const size_t rescued = eng.RescuedWalkers();
    eng.WarmUp();
    std::copy(comp.config.data(), comp.config.data() + (size_t)n * rows * cols, configs);
    std::copy(sitps.flat().begin(), sitps.flat().end(), sitps_flat);
    copy_out(comp.amplitude, amplitudes_out);
    out[0] = eng.LastScaleFactor(); out[1] = (double)rescued; out[2] = eng.IsWarmedUp() ? 1.0 : 0.0;
  });
}
int pepshost_mc_engine_warmup(int rows, int cols, int D, int d, int chi, int dtype, double *sitps_flat, int n, int32_t *configs,
                              const uint64_t *seeds, int warmup_sweeps, int rescue_enabled, double amp_min, double amp_max,
                              double *amplitudes_out, double *out) {
  return mc_engine_warmup_impl(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, seeds, warmup_sweeps, rescue_enabled, amp_min, amp_max,
                               amplitudes_out, out, nullptr, nullptr);
}
// Several ranks (one process per GPU): max_over_ranks = the MPI_Allreduce(MAX) of NormalizeStateOrder1 (monte_carlo_engine.h:214-222),
// exchange_valid_config = the MPI_Allgather + MPI_BCast of EnsureConfigurationValidity (:344-387) -- both supplied by the caller
// (peps_amd/dist.py over torch.distributed); either may be NULL.
int pepshost_mc_engine_warmup_dist(int rows, int cols, int D, int d, int chi, int dtype, double *sitps_flat, int n, int32_t *configs,
                                   const uint64_t *seeds, int warmup_sweeps, int rescue_enabled, double amp_min, double amp_max,
                                   double *amplitudes_out, double *out, double (*max_over_ranks)(double),
                                   int (*exchange_valid_config)(int, int, int32_t *)) {
  return mc_engine_warmup_impl(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, seeds, warmup_sweeps, rescue_enabled, amp_min, amp_max,
                               amplitudes_out, out, max_over_ranks, exchange_valid_config);
}

// CalEnergyAndHoles (model_energy_solver.h:32-126) for n configurations; model 0 = XXZ (p = jz, jxy,
// pinning00), 1 = TFIM (p[0] = h).  holes_out (nullable) = [n][rows][cols][D^4]; psi_out = [n_psi][n].
int pepshost_energy_and_holes(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n,
                              const int32_t *configs, int model, const double *p, double *amplitudes_out,
                              double *energies_out, double *holes_out, double *psi_out, int *n_psi_out) {
  return guarded([&]() {
    energy_and_holes_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, model, p, amplitudes_out, energies_out, holes_out,
                                  psi_out, n_psi_out);
  });
}
// the same for TenElemT = QLTEN_Complex: sitps_flat and every output scalar / tensor = interleaved (re, im) pairs
int pepshost_energy_and_holes_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n,
                                   const int32_t *configs, int model, const double *p, double *amplitudes_out,
                                   double *energies_out, double *holes_out, double *psi_out, int *n_psi_out) {
  return guarded([&]() {
    energy_and_holes_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, n, configs, model, p, amplitudes_out, energies_out,
                                         holes_out, psi_out, n_psi_out);
  });
}

// Rank-local part of MCEnergyGradEvaluator::Evaluate (mc_energy_grad_evaluator.h:205-310): warm-up
// sweeps, then n_samples x {one MC sweep, CalEnergyAndHoles, O* accumulation}; the holes and the
// tensor sums stay on the device.  packed_out as in pepshost_exact_sum_partial (weight 1 per sample);
// the caller all-reduces it over ranks and calls pepshost_exact_sum_finish.
int pepshost_mc_energy_grad_partial(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n,
                                    int32_t *configs, const uint64_t *seeds, int updater, int model, const double *p,
                                    int warmup_sweeps, int n_samples, double *packed_out, double *accept_out) {
  return guarded([&]() {
    mc_energy_grad_partial_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, seeds, updater, model, p, warmup_sweeps,
                                        n_samples, packed_out, accept_out);
  });
}
// QLTEN_Complex: packed_out = [S_O | S_EO (interleaved pairs) | sum w | Re, Im sum wE | sum w|E|^2 | samples], 4 m + 5 doubles
int pepshost_mc_energy_grad_partial_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n,
                                         int32_t *configs, const uint64_t *seeds, int updater, int model, const double *p,
                                         int warmup_sweeps, int n_samples, double *packed_out, double *accept_out) {
  return guarded([&]() {
    mc_energy_grad_partial_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, n, configs, seeds, updater, model, p,
                                               warmup_sweeps, n_samples, packed_out, accept_out);
  });
}

// EvaluateObservables of the XXZ (model 0) / TFIM (model 1, p[0] = h) / J1-J2 (model 2) / triangular J1-J2 (model 4, p[0] = j2) measurement solver on fixed configurations, or -- with
// n_samples > 0 -- a whole MCPEPSMeasurer run (warm-up, samples, statistics across the walkers, optional DumpData).
// Results come back through a flat buffer described by `keys_out` ("key:len;key:len;..."): for n_samples == 0 the
// per-walker values [key][walker][len], else [key][mean(len) | stderr(len)], followed by psi_mean[n], psi_rel_err[n]
// of the last sample.
int pepshost_measure(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, int32_t *configs,
                     const uint64_t *seeds, int updater, int model, const double *p, int warmup_sweeps, int n_samples,
                     int sweeps_between_samples, const char *dump_dir, char *keys_out, int keys_cap, double *values_out,
                     long values_cap, long *values_len) {
  return guarded([&]() {
    measure_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, seeds, updater, model, p, warmup_sweeps, n_samples,
                         sweeps_between_samples, dump_dir, keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
// QLTEN_Complex (ObservableMap<TenElemT> of the reference is complex for a complex state): sitps_flat and every number of values_out --
// observables, standard errors, psi_mean, psi_rel_err -- are interleaved (re, im) pairs; values_len counts doubles.
int pepshost_measure_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n, int32_t *configs,
                          const uint64_t *seeds, int updater, int model, const double *p, int warmup_sweeps, int n_samples,
                          int sweeps_between_samples, const char *dump_dir, char *keys_out, int keys_cap, double *values_out,
                          long values_cap, long *values_len) {
  return guarded([&]() {
    measure_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, n, configs, seeds, updater, model, p, warmup_sweeps, n_samples,
                                sweeps_between_samples, dump_dir, keys_out, keys_cap, values_out, values_cap, values_len);
  });
}

// Rank-local part of ExactSumEnergyEvaluatorMPI (exact_summation_energy_evaluator.h:173-245):
// packed_out = [S_O | S_EO | sum w | sum wE | sum wE^2 | samples], length 2*rows*cols*d*D^4 + 4.
int pepshost_exact_sum_partial(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat,
                               const int32_t *all_configs, int n_configs, int model, const double *p, int rank, int size,
                               int batch, double *packed_out) {
  return guarded([&]() {
    exact_sum_partial_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, all_configs, n_configs, model, p, rank, size, batch, packed_out);
  });
}
// QLTEN_Complex (layout of packed_out: see pepshost_mc_energy_grad_partial_c128)
int pepshost_exact_sum_partial_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat,
                                    const int32_t *all_configs, int n_configs, int model, const double *p, int rank, int size,
                                    int batch, double *packed_out) {
  return guarded([&]() {
    exact_sum_partial_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, all_configs, n_configs, model, p, rank, size, batch,
                                          packed_out);
  });
}

// Rank-local part of ExactSumMeasurerMPI (exact_summation_measurer.h:103-257): un-normalised weighted sums of the
// registry observables over configurations rank, rank + size, ...   keys_out = "key:len;...", values_out =
// [sum w | key values in that order]; the caller sums values over ranks and divides by values[0].
// n_configs < 0: every binary configuration (GenerateAllBinaryConfigs).
int pepshost_exact_sum_measure_partial(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat,
                                       const int32_t *all_configs, int n_configs, int model, const double *p, int rank, int size,
                                       int batch, char *keys_out, int keys_cap, double *values_out, long values_cap, long *values_len) {
  return guarded([&]() {
    exact_sum_measure_partial_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, all_configs, n_configs, model, p, rank, size, batch,
                                           keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
// QLTEN_Complex: values_out = [sum w (one double) | key values as (re, im) pairs]
int pepshost_exact_sum_measure_partial_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat,
                                            const int32_t *all_configs, int n_configs, int model, const double *p, int rank, int size,
                                            int batch, char *keys_out, int keys_cap, double *values_out, long values_cap, long *values_len) {
  return guarded([&]() {
    exact_sum_measure_partial_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, all_configs, n_configs, model, p, rank, size,
                                                  batch, keys_out, keys_cap, values_out, values_cap, values_len);
  });
}

// Optimizer::IterativeOptimize + exact summation on the device (see optimize_exact_sum_impl)
int pepshost_optimize_exact_sum(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, const int32_t *all_configs,
                                int n_configs, int model, const double *p, int rule, double lr, const double *rule_params, int n_rule_params,
                                int iterations, double clip_value, double clip_norm, int batch, double *energies_out, double *grad_norms_out,
                                double *state_out) {
  return guarded([&]() {
    optimize_exact_sum_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, all_configs, n_configs, model, p, rule, lr, rule_params,
                                    n_rule_params, iterations, clip_value, clip_norm, batch, energies_out, grad_norms_out, state_out);
  });
}
// QLTEN_Complex: sitps_flat, energies_out and state_out are interleaved (re, im) pairs
int pepshost_optimize_exact_sum_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, const int32_t *all_configs,
                                     int n_configs, int model, const double *p, int rule, double lr, const double *rule_params,
                                     int n_rule_params, int iterations, double clip_value, double clip_norm, int batch, double *energies_out,
                                     double *grad_norms_out, double *state_out) {
  return guarded([&]() {
    optimize_exact_sum_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, all_configs, n_configs, model, p, rule, lr,
                                           rule_params, n_rule_params, iterations, clip_value, clip_norm, batch, energies_out,
                                           grad_norms_out, state_out);
  });
}
// Optimizer's SR step on a given sample set (see sr_step_samples_impl)
int pepshost_sr_step_samples(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, const int32_t *configs,
                             int model, const double *p, double lr, double diag_shift, int cg_max_iter, double cg_relative_tolerance,
                             int normalize_update, double *state_out, double *info_out) {
  return guarded([&]() {
    sr_step_samples_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, model, p, lr, diag_shift, cg_max_iter,
                                 cg_relative_tolerance, normalize_update, state_out, info_out);
  });
}
int pepshost_sr_step_samples_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n, const int32_t *configs,
                                  int model, const double *p, double lr, double diag_shift, int cg_max_iter, double cg_relative_tolerance,
                                  int normalize_update, double *state_out, double *info_out) {
  return guarded([&]() {
    sr_step_samples_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, n, configs, model, p, lr, diag_shift, cg_max_iter,
                                        cg_relative_tolerance, normalize_update, state_out, info_out);
  });
}
// Optimizer's MinSR step on a given sample set (see minsr_step_samples_impl)
int pepshost_minsr_step_samples(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, const int32_t *configs,
                                int model, const double *p, double lr, double r_pinv, double a_pinv, int soft_cutoff, int exact_sum,
                                double *state_out, double *info_out) {
  return guarded([&]() {
    minsr_step_samples_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, n, configs, model, p, lr, r_pinv, a_pinv, soft_cutoff, exact_sum,
                                    state_out, info_out);
  });
}
int pepshost_minsr_step_samples_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n, const int32_t *configs,
                                     int model, const double *p, double lr, double r_pinv, double a_pinv, int soft_cutoff, int exact_sum,
                                     double *state_out, double *info_out) {
  return guarded([&]() {
    minsr_step_samples_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, n, configs, model, p, lr, r_pinv, a_pinv,
                                           soft_cutoff, exact_sum, state_out, info_out);
  });
}
// Optimizer::IterativeOptimize with LBFGSParams + exact summation (see lbfgs_exact_sum_impl)
int pepshost_lbfgs_exact_sum(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, const int32_t *all_configs,
                             int n_configs, int model, const double *p, double lr, const double *lbfgs, int iterations,
                             double energy_tolerance, double gradient_tolerance, int plateau_patience, int batch, double *energies_out,
                             double *grad_norms_out, double *steps_out, double *state_out, double *info_out) {
  return guarded([&]() {
    lbfgs_exact_sum_impl<double>(rows, cols, D, d, chi, dtype, sitps_flat, all_configs, n_configs, model, p, lr, lbfgs, iterations,
                                 energy_tolerance, gradient_tolerance, plateau_patience, batch, energies_out, grad_norms_out, steps_out,
                                 state_out, info_out);
  });
}
int pepshost_lbfgs_exact_sum_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, const int32_t *all_configs,
                                  int n_configs, int model, const double *p, double lr, const double *lbfgs, int iterations,
                                  double energy_tolerance, double gradient_tolerance, int plateau_patience, int batch,
                                  double *energies_out, double *grad_norms_out, double *steps_out, double *state_out, double *info_out) {
  return guarded([&]() {
    lbfgs_exact_sum_impl<QLTEN_Complex>(rows, cols, D, d, chi, PEPSGPU_C128, sitps_flat, all_configs, n_configs, model, p, lr, lbfgs,
                                        iterations, energy_tolerance, gradient_tolerance, plateau_patience, batch, energies_out,
                                        grad_norms_out, steps_out, state_out, info_out);
  });
}
int pepshost_fermion_lbfgs_exact_sum(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                     const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model, const double *prm,
                                     int n_prm, double lr, const double *lbfgs, int iterations, double energy_tolerance,
                                     double gradient_tolerance, int plateau_patience, int batch, double *energies_out,
                                     double *grad_norms_out, double *steps_out, double *state_out, double *info_out) {
  return guarded([&]() {
    fermion_lbfgs_exact_sum_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, prm,
                                         n_prm, lr, lbfgs, iterations, energy_tolerance, gradient_tolerance, plateau_patience, batch,
                                         energies_out, grad_norms_out, steps_out, state_out, info_out);
  });
}
int pepshost_fermion_lbfgs_exact_sum_c128(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi,
                                          const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model,
                                          const double *prm, int n_prm, double lr, const double *lbfgs, int iterations,
                                          double energy_tolerance, double gradient_tolerance, int plateau_patience, int batch,
                                          double *energies_out, double *grad_norms_out, double *steps_out, double *state_out,
                                          double *info_out) {
  return guarded([&]() {
    fermion_lbfgs_exact_sum_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, PEPSGPU_C128, sitps_ext_flat, all_configs,
                                                n_configs, model, prm, n_prm, lr, lbfgs, iterations, energy_tolerance, gradient_tolerance,
                                                plateau_patience, batch, energies_out, grad_norms_out, steps_out, state_out, info_out);
  });
}
// Optimizer::IterativeOptimize + exact summation on a fermionic state (see fermion_optimize_exact_sum_impl)
int pepshost_fermion_optimize_exact_sum(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                        const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model,
                                        const double *prm, int n_prm, int rule, double lr, const double *rule_params, int n_rule_params,
                                        int iterations, double clip_value, double clip_norm, int batch, double *energies_out,
                                        double *grad_norms_out, double *state_out) {
  return guarded([&]() {
    fermion_optimize_exact_sum_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, prm,
                                            n_prm, rule, lr, rule_params, n_rule_params, iterations, clip_value, clip_norm, batch,
                                            energies_out, grad_norms_out, state_out);
  });
}
int pepshost_fermion_optimize_exact_sum_c128(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi,
                                             const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model,
                                             const double *prm, int n_prm, int rule, double lr, const double *rule_params,
                                             int n_rule_params, int iterations, double clip_value, double clip_norm, int batch,
                                             double *energies_out, double *grad_norms_out, double *state_out) {
  return guarded([&]() {
    fermion_optimize_exact_sum_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, PEPSGPU_C128, sitps_ext_flat, all_configs,
                                                   n_configs, model, prm, n_prm, rule, lr, rule_params, n_rule_params, iterations,
                                                   clip_value, clip_norm, batch, energies_out, grad_norms_out, state_out);
  });
}
// Optimizer's SR step on a given sample set of a fermionic state (see fermion_sr_step_samples_impl)
int pepshost_fermion_sr_step_samples(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                     const double *sitps_ext_flat, int n, const int32_t *configs, int model, const double *prm, int n_prm,
                                     double lr, double diag_shift, int cg_max_iter, double cg_relative_tolerance, int normalize_update,
                                     double *state_out, double *info_out) {
  return guarded([&]() {
    fermion_sr_step_samples_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_ext_flat, n, configs, model, prm, n_prm, lr,
                                         diag_shift, cg_max_iter, cg_relative_tolerance, normalize_update, state_out, info_out);
  });
}
int pepshost_fermion_sr_step_samples_c128(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi,
                                          const double *sitps_ext_flat, int n, const int32_t *configs, int model, const double *prm,
                                          int n_prm, double lr, double diag_shift, int cg_max_iter, double cg_relative_tolerance,
                                          int normalize_update, double *state_out, double *info_out) {
  return guarded([&]() {
    fermion_sr_step_samples_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, PEPSGPU_C128, sitps_ext_flat, n, configs, model, prm,
                                                n_prm, lr, diag_shift, cg_max_iter, cg_relative_tolerance, normalize_update, state_out,
                                                info_out);
  });
}

// LearningRateScheduler::GetLearningRate (lr_schedulers.h:40-103): kind 0 ConstantLR (lr), 1 ExponentialDecayLR (initial_lr, decay_rate,
// decay_steps), 2 StepLR (initial_lr, step_size, gamma)
// ---- Monte-Carlo VMC on the resident state (see vmc_optimize_impl / mc_evaluate_resident_impl) ----
// mc = [warmup_sweeps, samples_per_walker, sweeps_between_samples]; opt = [algo, lr, iterations, clip_value, clip_norm, finalize,
// probe_iteration]
static VMCSpec vmc_spec(const double *mc, const double *opt, const double *rule_params, int n_rule_params) {
  if (!mc || !opt) throw std::invalid_argument("vmc: the mc / opt arrays are required");
  for (int i = 0; i < 3; ++i) if (!(mc[i] >= 0.0 && mc[i] < 1e9)) throw std::invalid_argument("vmc: sweeps / samples out of range");
  if (!(opt[2] >= 0.0 && opt[2] < 1e9)) throw std::invalid_argument("vmc: iterations out of range");
  VMCSpec v;
  v.warmup_sweeps = (int)mc[0]; v.samples_per_walker = (int)mc[1]; v.sweeps_between = (int)mc[2];
  v.algo = (int)opt[0]; v.lr = opt[1]; v.iterations = (int)opt[2]; v.clip_value = opt[3]; v.clip_norm = opt[4];
  v.rule_params = rule_params; v.n_rule_params = n_rule_params;
  return v;
}
int pepshost_vmc_optimize(int rows, int cols, int D, int d, int chi, int dtype, const double *sitps_flat, int n, int32_t *configs,
                          const uint64_t *seeds, int n_seeds, int updater, int model, const double *p, const double *mc, const double *opt,
                          const double *rule_params, int n_rule_params, const char *tps_base, const char *energy_dir, const char *config_dir,
                          double *energies_out, double *errors_out, double *grad_norms_out, double *accept_out, double *state_out,
                          double *lowest_out, double *probe_state_out, double *info_out) {
  return guarded([&]() {
    const VMCSpec v = vmc_spec(mc, opt, rule_params, n_rule_params);
    vmc_optimize_impl<double>(rows, cols, D, d, nullptr, nullptr, chi, dtype, sitps_flat, n, configs, seeds, n_seeds, updater, model, p, 8, v,
                              (int)opt[5], (int)opt[6], tps_base, energy_dir, config_dir, energies_out, errors_out, grad_norms_out, accept_out,
                              state_out, lowest_out, probe_state_out, info_out);
  });
}
// QLTEN_Complex: sitps_flat, energies_out and the states are interleaved (re, im) pairs
int pepshost_vmc_optimize_c128(int rows, int cols, int D, int d, int chi, const double *sitps_flat, int n, int32_t *configs,
                               const uint64_t *seeds, int n_seeds, int updater, int model, const double *p, const double *mc,
                               const double *opt, const double *rule_params, int n_rule_params, const char *tps_base, const char *energy_dir,
                               const char *config_dir, double *energies_out, double *errors_out, double *grad_norms_out, double *accept_out,
                               double *state_out, double *lowest_out, double *probe_state_out, double *info_out) {
  return guarded([&]() {
    const VMCSpec v = vmc_spec(mc, opt, rule_params, n_rule_params);
    vmc_optimize_impl<QLTEN_Complex>(rows, cols, D, d, nullptr, nullptr, chi, PEPSGPU_C128, sitps_flat, n, configs, seeds, n_seeds, updater,
                                     model, p, 8, v, (int)opt[5], (int)opt[6], tps_base, energy_dir, config_dir, energies_out, errors_out,
                                     grad_norms_out, accept_out, state_out, lowest_out, probe_state_out, info_out);
  });
}
// a fermionic state: sitps_ext_flat = the 4 d decorated components, bond_parity [rows][cols][4][D]; the states come back as the d stored
// components; dtype PEPSGPU_C128 runs the QLTEN_Complex instantiation
int pepshost_fermion_vmc_optimize(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                  const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int n_seeds, int updater,
                                  int model, const double *prm, int n_prm, const double *mc, const double *opt, const double *rule_params,
                                  int n_rule_params, const char *tps_base, const char *energy_dir, const char *config_dir,
                                  double *energies_out, double *errors_out, double *grad_norms_out, double *accept_out, double *state_out,
                                  double *lowest_out, double *probe_state_out, double *info_out) {
  return guarded([&]() {
    if (!nf || !bond_parity) throw std::invalid_argument("pepshost_fermion_vmc_optimize: nf and bond_parity are required");
    const VMCSpec v = vmc_spec(mc, opt, rule_params, n_rule_params);
    if (dtype == PEPSGPU_C128)
      vmc_optimize_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_ext_flat, n, configs, seeds, n_seeds, updater, model,
                                       prm, n_prm, v, (int)opt[5], (int)opt[6], tps_base, energy_dir, config_dir, energies_out, errors_out,
                                       grad_norms_out, accept_out, state_out, lowest_out, probe_state_out, info_out);
    else
      vmc_optimize_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_ext_flat, n, configs, seeds, n_seeds, updater, model, prm,
                                n_prm, v, (int)opt[5], (int)opt[6], tps_base, energy_dir, config_dir, energies_out, errors_out, grad_norms_out,
                                accept_out, state_out, lowest_out, probe_state_out, info_out);
  });
}
// nf == NULL: a bosonic state; dtype PEPSGPU_C128 runs the QLTEN_Complex instantiation.  opt may be NULL (no step).
int pepshost_mc_evaluate_resident(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                  const double *sitps_flat, int n, int32_t *configs, const uint64_t *seeds, int updater, int model,
                                  const double *p, int n_prm, int warmup_sweeps, int normalize, int n_samples, int n_evaluates,
                                  int collect_sr, const double *opt, const double *rule_params, int n_rule_params,
                                  double *energy_samples_out, double *so_out, double *seo_out, double *scalars_out, double *accept_out,
                                  double *state_out, double *step_info_out) {
  return guarded([&]() {
    VMCSpec v;
    v.algo = -1;
    if (opt) { v.algo = (int)opt[0]; v.lr = opt[1]; v.clip_value = opt[3]; v.clip_norm = opt[4]; v.rule_params = rule_params; v.n_rule_params = n_rule_params; }
    if (dtype == PEPSGPU_C128)
      mc_evaluate_resident_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_flat, n, configs, seeds, updater, model, p,
                                               n_prm, warmup_sweeps, normalize, n_samples, n_evaluates, collect_sr, v, energy_samples_out,
                                               so_out, seo_out, scalars_out, accept_out, state_out, step_info_out);
    else
      mc_evaluate_resident_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_flat, n, configs, seeds, updater, model, p, n_prm,
                                        warmup_sweeps, normalize, n_samples, n_evaluates, collect_sr, v, energy_samples_out, so_out, seo_out,
                                        scalars_out, accept_out, state_out, step_info_out);
  });
}
// MeanAndBinnedErrorSqrtNUniformBin on a host array samples [n_samples][n_walkers] (interleaved pairs when is_complex); no device.
// mean_out: 1 or 2 doubles.
int pepshost_binned_energy_stat(const double *samples, int n_samples, int n_walkers, int is_complex, double *mean_out, double *err_out) {
  return guarded([&]() {
    if (!samples || !mean_out || !err_out || n_samples < 0 || n_walkers < 1) throw std::invalid_argument("pepshost_binned_energy_stat: bad arguments");
    const size_t cnt = (size_t)n_samples * n_walkers;
    if (is_complex) {
      const QLTEN_Complex *src = reinterpret_cast<const QLTEN_Complex *>(samples);
      const auto r = MeanAndBinnedErrorSqrtNUniformBin(std::vector<QLTEN_Complex>(src, src + cnt), (size_t)n_walkers);
      mean_out[0] = r.first.real(); mean_out[1] = r.first.imag(); *err_out = r.second;
    } else {
      const auto r = MeanAndBinnedErrorSqrtNUniformBin(std::vector<double>(samples, samples + cnt), (size_t)n_walkers);
      mean_out[0] = r.first; *err_out = r.second;
    }
  });
}

// ---- spike recovery and step selectors: the decision code alone, on the host (no device) ----
// EMATracker over series[n]: mean_out / var_out after every Update; reset_at >= 0: Reset() before that observation
int pepshost_ema_track(const double *series, int n, long window, int reset_at, double *mean_out, double *var_out) {
  return guarded([&]() {
    if (!series || !mean_out || !var_out || n < 0 || window < 0) throw std::invalid_argument("pepshost_ema_track: bad arguments");
    EMATracker t((size_t)window);
    for (int i = 0; i < n; ++i) {
      if (i == reset_at) {
        t.Reset();
        if (t.IsInitialized() || t.Mean() != 0.0 || t.Var() != 0.0) throw std::logic_error("pepshost_ema_track: Reset left state behind");
      }
      t.Update(series[i]);
      mean_out[i] = t.Mean(); var_out[i] = t.Var();
    }
  });
}
// The SpikeGuard of Optimizer::IterativeOptimize driven by a scripted series: records [n][5] = (energy, error, grad_norm, ngrad_norm,
// cg_iters), one per evaluation in the order the optimizer would make them; algo as make_vmc_algo (3 SR: S3 with the CG iterations,
// 4 MinSR: S3 on the norm only, others: no S3).  guard: the nine spike fields.  A rejected record (resample, rollback) is followed by
// the next record at the same iteration.  actions_out [n]: the verdict per record (SpikeAction; accepted with a warning = 3);
// iters_out [n]: the iteration it was judged at; ema_out [n][8]: mean and var of the four trackers after the record; events_out
// [cap][6] and counts_out [4] as write_events; csv_out (cap csv_cap): the trigger CSV of the event log.
int pepshost_spike_replay(const double *records, int n, int algo, const double *guard, int32_t *actions_out, int32_t *iters_out,
                          double *ema_out, double *events_out, int events_cap, double *counts_out, char *csv_out, long csv_cap) {
  return guarded([&]() {
    if (!records || n < 0 || !guard || !actions_out || events_cap < 0) throw std::invalid_argument("pepshost_spike_replay: bad arguments");
    SpikeGuard sg(make_spike_params(guard, nullptr), /*log_to_stdout=*/false);
    const bool is_sr = algo == 3, is_minsr = algo == 4;
    size_t iter = 0, attempts = 0;
    for (int k = 0; k < n; ++k) {
      const double *r = records + 5 * (size_t)k;
      if (iters_out) iters_out[k] = (int32_t)iter;
      bool warned = false;
      auto rejected = [&](SpikeAction a) {
        if (a == SpikeAction::kAcceptWithWarning) warned = true;
        if (a == SpikeAction::kResample) { ++attempts; return true; }
        if (a == SpikeAction::kRollback) { sg.TakeBase(); attempts = 0; return true; }
        return false;
      };
      SpikeAction a = sg.JudgeEvaluation(iter, attempts, r[1], r[2]);
      bool out = rejected(a);
      if (!out && (is_sr || is_minsr) && sg.Params().enable_auto_recover) {
        a = sg.JudgeDirection(iter, attempts, r[3], is_minsr ? std::numeric_limits<size_t>::max() : (size_t)r[4]);
        out = rejected(a);
      }
      if (!out) { a = sg.JudgeEnergy(iter, attempts, r[0]); out = rejected(a); }
      if (!out) {
        sg.Accept(r[0], r[1], r[2], (is_sr || is_minsr) ? r + 3 : nullptr);
        if (sg.Params().enable_rollback) sg.MarkBaseSaved();
        a = warned ? SpikeAction::kAcceptWithWarning : SpikeAction::kAccept;
        ++iter; attempts = 0;
      }
      actions_out[k] = (int32_t)a;
      if (ema_out) {
        double *o = ema_out + 8 * (size_t)k;
        const EMATracker *t[4] = {&sg.EnergyEMA(), &sg.ErrorEMA(), &sg.GradNormEMA(), &sg.NaturalGradNormEMA()};
        for (int j = 0; j < 4; ++j) { o[2 * j] = t[j]->Mean(); o[2 * j + 1] = t[j]->Var(); }
      }
    }
    write_events(sg.Statistics(), (size_t)events_cap, events_out, counts_out);
    if (csv_out && csv_cap > 0) {
      std::ostringstream os;
      SpikeGuard::WriteTriggerCsv(os, sg.Statistics());
      const std::string t = os.str();
      if ((long)t.size() + 1 > csv_cap) throw std::out_of_range("pepshost_spike_replay: csv_out too small");
      std::memcpy(csv_out, t.c_str(), t.size() + 1);
    }
  });
}
// AcceptanceRateCheck: flags_out[w] = 1 for a walker whose rate is below half the maximum over the walkers
int pepshost_acceptance_rate_check(const double *rates, int n, int32_t *flags_out) {
  return guarded([&]() {
    if (n < 0 || (n > 0 && (!rates || !flags_out))) throw std::invalid_argument("pepshost_acceptance_rate_check: bad arguments");
    std::fill(flags_out, flags_out + n, 0);
    for (const size_t w : AcceptanceRateCheck(std::vector<double>(rates, rates + n))) flags_out[w] = 1;
  });
}
// The selection rule of a step selector: kind 0 initial, 1 periodic; results [n][3] = (eta, energy, error) of the trials;
// out = [selected eta, the selector's base learning rate afterwards].  Non-finite trial values throw as in the optimizer.
int pepshost_step_select(int kind, const double *results, int n, long iter, long max_iterations, double base_lr, double phase_switch_ratio,
                         double *out) {
  return guarded([&]() {
    if ((kind != 0 && kind != 1) || !results || !out || iter < 0 || max_iterations < 0) throw std::invalid_argument("pepshost_step_select: bad arguments");
    if (n < 1 || (kind == 1 && n != 2)) throw std::invalid_argument("pepshost_step_select: the initial rule takes >= 1 trials, the periodic rule 2");
    std::vector<StepCandidateResult> r;
    for (int i = 0; i < n; ++i) {
      CheckStepCandidate(results[3 * i + 1], results[3 * i + 2]);
      r.push_back({results[3 * i], results[3 * i + 1], results[3 * i + 2]});
    }
    out[0] = kind == 0 ? SelectInitialStep(r) : SelectPeriodicStep(r, (size_t)iter, (size_t)max_iterations, phase_switch_ratio);
    out[1] = NextSelectorBaseLR(kind == 0, base_lr, out[0]);
  });
}
// the candidates a selector tries from base_lr: kind 0 -> base_lr * 1 .. max_line_search_steps, kind 1 -> (base_lr, base_lr / 2)
int pepshost_step_candidates(int kind, double base_lr, int max_line_search_steps, double *out, int cap, int *n_out) {
  return guarded([&]() {
    if ((kind != 0 && kind != 1) || !out || !n_out || max_line_search_steps < 0) throw std::invalid_argument("pepshost_step_candidates: bad arguments");
    const std::vector<double> c = StepCandidates(kind == 0, base_lr, (size_t)max_line_search_steps);
    if ((int)c.size() > cap) throw std::out_of_range("pepshost_step_candidates: out too small");
    std::copy(c.begin(), c.end(), out);
    *n_out = (int)c.size();
  });
}
// OptimizerParams::ValidateGuards and VMCPEPSOptimizerParams::Validate for (algo, guard) with no device: what the guarded entries
// below refuse first.  n_walkers < 0: the optimizer's check alone.
int pepshost_validate_guards(int algo, const double *rule_params, int n_rule_params, double lr, const double *guard, int n_walkers, int n_seeds,
                             int samples_per_walker) {
  return guarded([&]() {
    VMCSpec v;
    v.algo = algo; v.rule_params = rule_params; v.n_rule_params = n_rule_params; v.lr = lr; v.samples_per_walker = samples_per_walker;
    GuardSpec gs;
    gs.g = guard;
    if (n_walkers < 0) { make_guarded_params(gs, 1, lr, 0.0, 0.0, make_vmc_algo(v)).ValidateGuards(); return; }
    VMCPEPSOptimizerParams vp = make_vmc_params(v, 8, "", "", "");
    vp.optimizer_params = make_guarded_params(gs, 1, lr, 0.0, 0.0, make_vmc_algo(v));
    vp.Validate((size_t)n_walkers, (size_t)n_seeds);
  });
}
// ---- ... and around the device-resident Optimizer (guarded_optimize_exact_sum_impl / guarded_vmc_optimize_impl) ----
// nf == NULL: a bosonic state; dtype PEPSGPU_C128 runs the QLTEN_Complex instantiation.  opt = [algo, lr, iterations, clip_value,
// clip_norm]; guard as GuardSpec; error_override / energy_shift [n_schedule] (n_schedule 0: no schedule).
int pepshost_guarded_optimize_exact_sum(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                        const double *sitps_flat, const int32_t *all_configs, int n_configs, int model, const double *prm,
                                        int n_prm, const double *opt, const double *rule_params, int n_rule_params, int batch,
                                        const double *guard, const char *csv_path, const char *checkpoint_path, const double *error_override,
                                        const double *energy_shift, int n_schedule, double *energies_out, double *errors_out,
                                        double *grad_norms_out, double *selected_eta_out, double *events_out, double *state_out,
                                        double *lowest_out, double *probe_state_out, double *info_out) {
  return guarded([&]() {
    if (!opt || !guard) throw std::invalid_argument("pepshost_guarded_optimize_exact_sum: the opt / guard arrays are required");
    if (!(opt[2] >= 0.0 && opt[2] < 1e9)) throw std::invalid_argument("pepshost_guarded_optimize_exact_sum: iterations out of range");
    VMCSpec v;
    v.algo = (int)opt[0]; v.lr = opt[1]; v.iterations = (int)opt[2]; v.clip_value = opt[3]; v.clip_norm = opt[4];
    v.rule_params = rule_params; v.n_rule_params = n_rule_params;
    GuardSpec gs;
    gs.g = guard; gs.csv_path = csv_path; gs.checkpoint_path = checkpoint_path; gs.error_override = error_override;
    gs.energy_shift = energy_shift; gs.n_schedule = n_schedule;
    if (dtype == PEPSGPU_C128)
      guarded_optimize_exact_sum_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_flat, all_configs, n_configs, model, prm,
                                                     n_prm, v, batch, gs, energies_out, errors_out, grad_norms_out, selected_eta_out, events_out,
                                                     state_out, lowest_out, probe_state_out, info_out);
    else
      guarded_optimize_exact_sum_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_flat, all_configs, n_configs, model, prm,
                                              n_prm, v, batch, gs, energies_out, errors_out, grad_norms_out, selected_eta_out, events_out,
                                              state_out, lowest_out, probe_state_out, info_out);
  });
}
int pepshost_guarded_vmc_optimize(int rows, int cols, int D, int d, const int32_t *nf, const uint8_t *bond_parity, int chi, int dtype,
                                  const double *sitps_flat, int n, int32_t *configs, const uint64_t *seeds, int n_seeds, int updater, int model,
                                  const double *prm, int n_prm, const double *mc, const double *opt, const double *rule_params,
                                  int n_rule_params, const double *guard, const char *csv_path, const char *checkpoint_path,
                                  const double *error_override, const double *energy_shift, int n_schedule, double *energies_out,
                                  double *errors_out, double *grad_norms_out, double *selected_eta_out, double *events_out, double *accept_out,
                                  double *state_out, double *lowest_out, double *info_out) {
  return guarded([&]() {
    if (!guard) throw std::invalid_argument("pepshost_guarded_vmc_optimize: the guard array is required");
    const VMCSpec v = vmc_spec(mc, opt, rule_params, n_rule_params);
    GuardSpec gs;
    gs.g = guard; gs.csv_path = csv_path; gs.checkpoint_path = checkpoint_path; gs.error_override = error_override;
    gs.energy_shift = energy_shift; gs.n_schedule = n_schedule;
    if (dtype == PEPSGPU_C128)
      guarded_vmc_optimize_impl<QLTEN_Complex>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_flat, n, configs, seeds, n_seeds, updater,
                                               model, prm, n_prm, v, gs, energies_out, errors_out, grad_norms_out, selected_eta_out, events_out,
                                               accept_out, state_out, lowest_out, info_out);
    else
      guarded_vmc_optimize_impl<double>(rows, cols, D, d, nf, bond_parity, chi, dtype, sitps_flat, n, configs, seeds, n_seeds, updater, model,
                                        prm, n_prm, v, gs, energies_out, errors_out, grad_norms_out, selected_eta_out, events_out, accept_out,
                                        state_out, lowest_out, info_out);
  });
}

int pepshost_lr_schedule(int kind, const double *args, int n_args, long iteration, double *lr_out) {
  return guarded([&]() {
    if (!args || !lr_out || iteration < 0) throw std::invalid_argument("pepshost_lr_schedule: null argument or negative iteration");
    static const int want[3] = {1, 3, 3};
    if (kind < 0 || kind > 2 || n_args != want[kind]) throw std::invalid_argument("pepshost_lr_schedule: kind 0 (1 argument), 1 (3), 2 (3)");
    std::unique_ptr<LearningRateScheduler> s;
    if (kind == 0) s = std::make_unique<ConstantLR>(args[0]);
    else if (kind == 1) {
      if (!(args[2] >= 1.0)) throw std::invalid_argument("pepshost_lr_schedule: decay_steps must be >= 1");
      s = std::make_unique<ExponentialDecayLR>(args[0], args[1], (size_t)args[2]);
    } else {
      if (!(args[1] >= 1.0)) throw std::invalid_argument("pepshost_lr_schedule: step_size must be >= 1");
      s = std::make_unique<StepLR>(args[0], (size_t)args[1], args[2]);
    }
    *lr_out = s->GetLearningRate((size_t)iteration, 0.0);
  });
}

// energy = sum wE / sum w, gradient = (S_EO - E S_O)/sum w   (:286-295) from the rank-summed accumulators
int pepshost_exact_sum_finish(int rows, int cols, int D, int d, const double *packed, double *energy_out, double *grad_out) {
  return guarded([&]() {
    SplitIndexTPS like(rows, cols, d, D);
    GradAccumulator acc(like);
    std::vector<double> v(packed, packed + 2 * like.flat().size() + 4);
    acc.Unpack(v);
    auto res = acc.Finish();
    *energy_out = res.first;
    std::copy(res.second.flat().begin(), res.second.flat().end(), grad_out);
  });
}

// QLTEN_Complex: packed = 4 m + 5 doubles (see pepshost_mc_energy_grad_partial_c128); energy_out = (re, im), grad_out = interleaved pairs
int pepshost_exact_sum_finish_c128(int rows, int cols, int D, int d, const double *packed, double *energy_out, double *grad_out) {
  return guarded([&]() {
    SplitIndexTPST<QLTEN_Complex> like(rows, cols, d, D);
    GradAccumulatorT<QLTEN_Complex> acc(like);
    std::vector<double> v(packed, packed + 4 * like.flat().size() + 5);
    acc.Unpack(v);
    auto res = acc.Finish();
    energy_out[0] = res.first.real(); energy_out[1] = res.first.imag();
    copy_out(res.second.flat(), grad_out);
  });
}
// SplitIndexTPS<QLTEN_Complex>::Load / Dump of the reference's complex fixtures (interleaved complex128 payloads)
int pepshost_load_sitps_c128(const char *dir, int D, int *rows, int *cols, int *d, double *flat_out, size_t flat_cap) {
  return guarded([&]() {
    auto s = SplitIndexTPST<QLTEN_Complex>::Load(dir, D);
    *rows = (int)s.rows(); *cols = (int)s.cols(); *d = (int)s.PhysicalDim();
    if (flat_out) {
      if (flat_cap < 2 * s.flat().size()) throw std::invalid_argument("output buffer too small");
      copy_out(s.flat(), flat_out);
    }
  });
}
int pepshost_dump_sitps_c128(const char *dir, int rows, int cols, int D, int d, const double *flat) {
  return guarded([&]() { make_state_t<QLTEN_Complex>(rows, cols, D, d, flat).Dump(dir); });
}

// SplitIndexTPS::Load round trip for the reference's dump format (dense fixtures)
int pepshost_load_sitps(const char *dir, int D, int *rows, int *cols, int *d, double *flat_out, size_t flat_cap) {
  return guarded([&]() {
    SplitIndexTPS s = SplitIndexTPS::Load(dir, D);
    *rows = (int)s.rows(); *cols = (int)s.cols(); *d = (int)s.PhysicalDim();
    if (flat_out) {
      if (flat_cap < s.flat().size()) throw std::invalid_argument("output buffer too small");
      std::copy(s.flat().begin(), s.flat().end(), flat_out);
    }
  });
}

// Fermionic state (extended, sign-decorated components: peps_amd/fermion.py): E_loc of the spinless t-V model and
// the amplitudes for a batch of physical configurations.  sitps_ext_flat has 4 * d components per site.
// model 0: spinless t-V (params t, V); model 1: t-J-V (params t, J, V, mu)
int pepshost_fermion_energy(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                            const double *sitps_ext_flat, int n, const int32_t *configs, int model, const double *prm,
                            double *amplitudes_out, double *energies_out, double *psi_out, int *n_psi_out) {
  return guarded([&]() {
    fermion_energy_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, prm, amplitudes_out, energies_out, psi_out,
                                n_psi_out);
  });
}
// QLTEN_Complex (SplitIndexTPS<QLTEN_Complex, fZ2QN>): the decorated components and every output as interleaved (re, im) pairs
int pepshost_fermion_energy_c128(int rows, int cols, int D, int d, const int32_t *nf, int chi,
                                 const double *sitps_ext_flat, int n, const int32_t *configs, int model, const double *prm,
                                 double *amplitudes_out, double *energies_out, double *psi_out, int *n_psi_out) {
  return guarded([&]() {
    fermion_energy_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, PEPSGPU_C128, sitps_ext_flat, n, configs, model, prm, amplitudes_out,
                                       energies_out, psi_out, n_psi_out);
  });
}

// ExactSumEnergyEvaluator on a fermionic state (spinless t-V): packed accumulators over the EXTENDED components
// (length 2 * rows*cols*4d*D^4 + 4); peps_amd.fermion.fold_gradient maps the finished gradient back
int pepshost_fermion_exact_sum_partial(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                       const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, double t,
                                       double V, int rank, int size, int batch, double *packed_out) {
  return guarded([&]() {
    fermion_exact_sum_partial_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, t, V, rank, size, batch,
                                           packed_out);
  });
}
// QLTEN_Complex: packed_out as pepshost_mc_energy_grad_partial_c128 (4 m + 5 doubles, m = rows*cols*4d*D^4); finish with
// pepshost_exact_sum_finish_c128 on d' = 4 d
int pepshost_fermion_exact_sum_partial_c128(int rows, int cols, int D, int d, const int32_t *nf, int chi,
                                            const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, double t,
                                            double V, int rank, int size, int batch, double *packed_out) {
  return guarded([&]() {
    fermion_exact_sum_partial_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, PEPSGPU_C128, sitps_ext_flat, all_configs, n_configs, t, V, rank,
                                                  size, batch, packed_out);
  });
}
// ... for either fermionic model (see fermion_exact_sum_partial_prm_impl); dtype PEPSGPU_C128 runs the complex instantiation
int pepshost_fermion_exact_sum_partial_prm(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                           const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model,
                                           const double *prm, int n_prm, int rank, int size, int batch, double *packed_out) {
  return guarded([&]() {
    if (dtype == PEPSGPU_C128)
      fermion_exact_sum_partial_prm_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, prm,
                                                        n_prm, rank, size, batch, packed_out);
    else
      fermion_exact_sum_partial_prm_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, prm, n_prm,
                                                 rank, size, batch, packed_out);
  });
}

// MCUpdateSquareNNExchangeOBC on a fermionic state: n_sweeps sweeps, configurations updated in place
int pepshost_fermion_mc_sweeps(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                               const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int n_sweeps,
                               double *amplitudes_out, double *accept_out) {
  return guarded([&]() {
    fermion_mc_sweeps_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, n_sweeps, amplitudes_out, accept_out);
  });
}
int pepshost_fermion_mc_sweeps_c128(int rows, int cols, int D, int d, const int32_t *nf, int chi,
                                    const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int n_sweeps,
                                    double *amplitudes_out, double *accept_out) {
  return guarded([&]() {
    fermion_mc_sweeps_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, PEPSGPU_C128, sitps_ext_flat, n, configs, seeds, n_sweeps, amplitudes_out,
                                          accept_out);
  });
}

// The same with the updater named: 0 = MCUpdateSquareNNExchangeOBC (as pepshost_fermion_mc_sweeps), 2 = MCUpdateSquareTNN3SiteExchange,
// 3 = MCUpdateSquareNNHubbardU1U1OBC; dtype PEPSGPU_C128 runs the complex instantiation (interleaved pairs)
int pepshost_fermion_mc_sweeps_updater(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                       const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int updater,
                                       int n_sweeps, double *amplitudes_out, double *accept_out) {
  return guarded([&]() {
    if (updater != 0 && updater != 2 && updater != 3)
      throw std::invalid_argument("pepshost_fermion_mc_sweeps_updater: updater must be 0 (exchange), 2 (tnn3) or 3 (hubbard_u1u1)");
    if (dtype == PEPSGPU_C128)
      fermion_mc_sweeps_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, n_sweeps, amplitudes_out,
                                            accept_out, updater);
    else
      fermion_mc_sweeps_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, n_sweeps, amplitudes_out, accept_out,
                                     updater);
  });
}

// The triple table of the three-site exchange (pepsgpu_sweep_slice_tnn3) on the host: nf == NULL -> bosonic, dp_or_d states per site,
// out [dp^3][20]; else fermionic, d = dp_or_d physical states of parities nf[d], over the 4 d extended states of mode order `order`
// (0 row-major, 1 column-major), out [(4 d)^3][20].
int pepshost_tnn3_table(int dp_or_d, const int32_t *nf, int order, int32_t *out) {
  return guarded([&]() {
    if (dp_or_d < 1 || dp_or_d > 64) throw std::invalid_argument("pepshost_tnn3_table: 1 <= states per site <= 64");
    if (order != 0 && order != 1) throw std::invalid_argument("pepshost_tnn3_table: order must be 0 (row-major) or 1 (column-major)");
    std::vector<int32_t> tab;
    if (nf) {
      FermionDecoration dec;
      dec.nf.assign(nf, nf + dp_or_d);
      tab = FermionTNN3Table(dec, order == 0 ? ROW_MAJOR : COL_MAJOR);
    } else {
      tab = TNN3TripleTable(dp_or_d);
    }
    std::copy(tab.begin(), tab.end(), out);
  });
}

// MCPEPSMeasurer's energy on a fermionic state with ONE random stream per walker over the whole run (monte_carlo_engine.h:146-176,
// monte_carlo_peps_measurer_impl.h:495-519): warmup_sweeps sweeps, the component rebuilt as NormalizeStateOrder1 does (the scale drops out
// of every ratio; the amplitude is evaluated afresh), then n_samples x {sweeps_between sweeps, E_loc}.  energies_out = [sample][walker].
// This is the call that reproduces the reference's fermionic regression value on the device (K9 of DESIGN 2: 6x6 fU1 t-J state, seed 42,
// -14.74320489110316; tests/test_gpu_fermion.py).
int pepshost_fermion_measure_energy(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                    const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int warmup_sweeps,
                                    int n_samples, int sweeps_between, int model, const double *prm, double *energies_out,
                                    double *accept_out) {
  return guarded([&]() {
    fermion_measure_energy_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples,
                                        sweeps_between, model, prm, energies_out, accept_out);
  });
}
int pepshost_fermion_measure_energy_c128(int rows, int cols, int D, int d, const int32_t *nf, int chi,
                                         const double *sitps_ext_flat, int n, int32_t *configs, const uint64_t *seeds, int warmup_sweeps,
                                         int n_samples, int sweeps_between, int model, const double *prm, double *energies_out,
                                         double *accept_out) {
  return guarded([&]() {
    fermion_measure_energy_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, PEPSGPU_C128, sitps_ext_flat, n, configs, seeds, warmup_sweeps,
                                               n_samples, sweeps_between, model, prm, energies_out, accept_out);
  });
}

// The two calls above with a parameter count, every element type in one entry (dtype PEPSGPU_C128: the complex instantiation, interleaved
// pairs): model 0 params [t, V, t2], model 1 [t, J, V, mu, t2] -- the t-t'-J model --, model 3 [t, U, mu] -- the Hubbard model (energy
// entry only); a shorter list leaves the missing parameters 0.
int pepshost_fermion_energy_prm(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat,
                                int n, const int32_t *configs, int model, int n_prm, const double *prm, double *amplitudes_out,
                                double *energies_out, double *psi_out, int *n_psi_out) {
  return guarded([&]() {
    if (n_prm < 0 || n_prm > 5 || (model != 0 && model != 1 && model != 3))
      throw std::invalid_argument("pepshost_fermion_energy_prm: model 0 / 1 / 3 (hubbard: [t, U, mu]), at most 5 parameters");
    double p[5] = {0, 0, 0, 0, 0};
    std::copy(prm, prm + n_prm, p);
    if (dtype == PEPSGPU_C128)
      fermion_energy_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, p, amplitudes_out, energies_out,
                                         psi_out, n_psi_out, 5);
    else
      fermion_energy_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, p, amplitudes_out, energies_out, psi_out,
                                  n_psi_out, 5);
  });
}
int pepshost_fermion_measure_energy_prm(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat,
                                        int n, int32_t *configs, const uint64_t *seeds, int warmup_sweeps, int n_samples, int sweeps_between,
                                        int model, int n_prm, const double *prm, double *energies_out, double *accept_out) {
  return guarded([&]() {
    if (n_prm < 0 || n_prm > 5 || (model != 0 && model != 1)) throw std::invalid_argument("pepshost_fermion_measure_energy_prm: model 0 / 1, at most 5 parameters");
    double p[5] = {0, 0, 0, 0, 0};
    std::copy(prm, prm + n_prm, p);
    if (dtype == PEPSGPU_C128)
      fermion_measure_energy_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples,
                                                 sweeps_between, model, p, energies_out, accept_out, 5);
    else
      fermion_measure_energy_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples,
                                          sweeps_between, model, p, energies_out, accept_out, 5);
  });
}

// The registry of the fermionic measurement solvers (SquareNNNModelMeasurementSolver on SquareSpinlessFermion / SquaretJVModel /
// SquaretJNNModel): energy, spin_z, charge, bond_energy_h / _v (/ _dr / _ur) and, for the t-J models, SC_bond_singlet_h / _v.  dtype
// PEPSGPU_C128 runs the complex instantiation; keys and values as pepshost_measure writes them.
// ... of a batch of configurations: per key [walker][len], then psi_mean [walker], psi_rel_err [walker]
int pepshost_fermion_observables(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat, int n,
                                 const int32_t *configs, int model, int n_prm, const double *prm, char *keys_out, int keys_cap,
                                 double *values_out, long values_cap, long *values_len) {
  return guarded([&]() {
    KeyedValues out;
    if (dtype == PEPSGPU_C128) fermion_observables_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, n_prm, prm, out);
    else fermion_observables_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, n_prm, prm, out);
    out.write("pepshost_fermion_observables", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
// ... summed with the weights |psi(S)|^2 over the configurations rank, rank + size, ... (ExactSumMeasurerMPI): values = [weight | sums]
int pepshost_fermion_exact_sum_measure_partial(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                               const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model, int n_prm,
                                               const double *prm, int rank, int size, int batch, char *keys_out, int keys_cap,
                                               double *values_out, long values_cap, long *values_len) {
  return guarded([&]() {
    KeyedValues out;
    if (dtype == PEPSGPU_C128)
      fermion_exact_sum_measure_partial_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, n_prm,
                                                            prm, rank, size, batch, out);
    else
      fermion_exact_sum_measure_partial_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, n_prm, prm,
                                                     rank, size, batch, out);
    out.write("pepshost_fermion_exact_sum_measure_partial", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
// ... sampled by MCPEPSMeasurer with the exchange updater: per key mean [len] and standard error [len] across the walkers, then the psi
// summary of the last sample; energy_samples_out [sample][walker] and accept_out [walker] may be NULL.  Warm-up, samples and ONE
// std::mt19937 stream per walker exactly as pepshost_fermion_measure_energy: the energy samples are that entry's.
int pepshost_fermion_measure(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat, int n,
                             int32_t *configs, const uint64_t *seeds, int warmup_sweeps, int n_samples, int sweeps_between, int model, int n_prm,
                             const double *prm, char *keys_out, int keys_cap, double *values_out, long values_cap, long *values_len,
                             double *energy_samples_out, double *accept_out) {
  return guarded([&]() {
    KeyedValues out;
    if (dtype == PEPSGPU_C128)
      fermion_measure_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples,
                                          sweeps_between, model, n_prm, prm, out, energy_samples_out, accept_out);
    else
      fermion_measure_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples, sweeps_between,
                                   model, n_prm, prm, out, energy_samples_out, accept_out);
    out.write("pepshost_fermion_measure", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}

// The same with the updater named: 0 = MCUpdateSquareNNExchangeOBC (pepshost_fermion_measure), 3 = MCUpdateSquareNNHubbardU1U1OBC
int pepshost_fermion_measure_updater(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat,
                                     int n, int32_t *configs, const uint64_t *seeds, int updater, int warmup_sweeps, int n_samples,
                                     int sweeps_between, int model, int n_prm, const double *prm, char *keys_out, int keys_cap,
                                     double *values_out, long values_cap, long *values_len, double *energy_samples_out, double *accept_out) {
  return guarded([&]() {
    KeyedValues out;
    if (dtype == PEPSGPU_C128)
      fermion_measure_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples,
                                          sweeps_between, model, n_prm, prm, out, energy_samples_out, accept_out, updater);
    else
      fermion_measure_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples, sweeps_between,
                                   model, n_prm, prm, out, energy_samples_out, accept_out, updater);
    out.write("pepshost_fermion_measure_updater", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
// The three entries above with SC_singlet_pair_corr of the t-J models (model 1 / 2; SingletPairCorrelationMixin): sc_pair_corr != 0
// enables it, ref_bonds [n_ref_bonds][2] = (y, x) of the left site of the selected reference bonds (n_ref_bonds == 0: all).  With
// sc_pair_corr == 0 they are the entries above.
int pepshost_fermion_observables_sc(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat, int n,
                                    const int32_t *configs, int model, int n_prm, const double *prm, char *keys_out, int keys_cap,
                                    double *values_out, long values_cap, long *values_len, int sc_pair_corr, int n_ref_bonds,
                                    const int32_t *ref_bonds) {
  return guarded([&]() {
    KeyedValues out;
    const SCPairArgs sc{sc_pair_corr, n_ref_bonds, ref_bonds};
    if (dtype == PEPSGPU_C128) fermion_observables_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, n_prm, prm, out, sc);
    else fermion_observables_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, model, n_prm, prm, out, sc);
    out.write("pepshost_fermion_observables_sc", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
int pepshost_fermion_exact_sum_measure_partial_sc(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype,
                                                  const double *sitps_ext_flat, const int32_t *all_configs, int n_configs, int model, int n_prm,
                                                  const double *prm, int rank, int size, int batch, char *keys_out, int keys_cap,
                                                  double *values_out, long values_cap, long *values_len, int sc_pair_corr, int n_ref_bonds,
                                                  const int32_t *ref_bonds) {
  return guarded([&]() {
    KeyedValues out;
    const SCPairArgs sc{sc_pair_corr, n_ref_bonds, ref_bonds};
    if (dtype == PEPSGPU_C128)
      fermion_exact_sum_measure_partial_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, n_prm,
                                                            prm, rank, size, batch, out, sc);
    else
      fermion_exact_sum_measure_partial_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, all_configs, n_configs, model, n_prm, prm,
                                                     rank, size, batch, out, sc);
    out.write("pepshost_fermion_exact_sum_measure_partial_sc", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
int pepshost_fermion_measure_sc(int rows, int cols, int D, int d, const int32_t *nf, int chi, int dtype, const double *sitps_ext_flat, int n,
                                int32_t *configs, const uint64_t *seeds, int warmup_sweeps, int n_samples, int sweeps_between, int model,
                                int n_prm, const double *prm, char *keys_out, int keys_cap, double *values_out, long values_cap,
                                long *values_len, double *energy_samples_out, double *accept_out, int sc_pair_corr, int n_ref_bonds,
                                const int32_t *ref_bonds) {
  return guarded([&]() {
    KeyedValues out;
    const SCPairArgs sc{sc_pair_corr, n_ref_bonds, ref_bonds};
    if (dtype == PEPSGPU_C128)
      fermion_measure_impl<QLTEN_Complex>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples,
                                          sweeps_between, model, n_prm, prm, out, energy_samples_out, accept_out, 0, sc);
    else
      fermion_measure_impl<double>(rows, cols, D, d, nf, chi, dtype, sitps_ext_flat, n, configs, seeds, warmup_sweeps, n_samples, sweeps_between,
                                   model, n_prm, prm, out, energy_samples_out, accept_out, 0, sc);
    out.write("pepshost_fermion_measure_sc", keys_out, keys_cap, values_out, values_cap, values_len);
  });
}
// GenerateSCPairCorrIndexMapping: out [n_pairs][6] = (ref_y, ref_x, 0, tgt_y, tgt_x, 0) in the order of the values; *n_pairs is set even
// when out is NULL or cap (in pairs) is too small (then nothing is written and the status is out of range); host only
int pepshost_sc_pair_corr_mapping(int rows, int cols, int n_ref_bonds, const int32_t *ref_bonds, int32_t *out, long cap, long *n_pairs) {
  return guarded([&]() {
    if (rows < 0 || cols < 0 || !n_pairs) throw std::invalid_argument("pepshost_sc_pair_corr_mapping: bad sizes or null count");
    const SCPairArgs sc{1, n_ref_bonds, ref_bonds};
    const auto mapping = SingletPairCorrelationMixin<SquaretJVModel>::GenerateSCPairCorrIndexMapping((size_t)rows, (size_t)cols,
                                                                                                      sc.selected("pepshost_sc_pair_corr_mapping"));
    *n_pairs = (long)mapping.size();
    if (!out) return;
    if ((long)mapping.size() > cap) throw std::out_of_range("pepshost_sc_pair_corr_mapping: output buffer too small");
    for (size_t i = 0; i < mapping.size(); ++i)
      for (size_t q = 0; q < 6; ++q) out[6 * i + q] = (int32_t)mapping[i][q];
  });
}
// The sector table of MCUpdateSquareNNHubbardU1U1OBC (pepsgpu_sweep_slice_sector), out [16][10]; host only
int pepshost_hubbard_sector_table(int32_t *out) {
  return guarded([&]() {
    if (!out) throw std::invalid_argument("pepshost_hubbard_sector_table: null output buffer");
    const std::vector<int32_t> tab = HubbardSectorTable();
    std::copy(tab.begin(), tab.end(), out);
  });
}
// The hop table of SquareHubbardModel (pepsgpu_nn_hop_slice_fermion), out [16][2][2]; host only
int pepshost_hubbard_hop_table(int32_t *out) {
  return guarded([&]() {
    if (!out) throw std::invalid_argument("pepshost_hubbard_hop_table: null output buffer");
    const std::vector<int32_t> tab = SquareHubbardModel::HopTable();
    std::copy(tab.begin(), tab.end(), out);
  });
}

// SplitIndexTPS::Dump (OBC leg dimensions) and the configuration{label} text files
int pepshost_dump_sitps(const char *dir, int rows, int cols, int D, int d, const double *flat) {
  return guarded([&]() {
    SplitIndexTPS s = make_state(rows, cols, D, d, flat);
    s.Dump(dir);
  });
}
int pepshost_dump_configuration(const char *dir, int label, int rows, int cols, const int32_t *config) {
  return guarded([&]() { DumpConfiguration(make_cfg(1, rows, cols, config), 0, dir, (size_t)label); });
}
// Configuration::Load (configuration.h:356-393): *loaded_out = 1 and the configuration in config_out, or *loaded_out = 0 (missing file, shape
// sidecar of another size, payload that does not parse) -- never an error code for those, as the reference never throws from Load.
// loaded_out == NULL: a configuration that cannot be loaded is an error (PEPSGPU_EEMPTY).
int pepshost_load_configuration2(const char *dir, int label, int rows, int cols, int32_t *config_out, int *loaded_out) {
  return guarded([&]() {
    Configuration c(1, rows, cols);
    const bool ok = LoadConfiguration(c, 0, dir, (size_t)label);
    if (loaded_out) *loaded_out = ok ? 1 : 0;
    else if (!ok) throw std::runtime_error(std::string("Configuration::Load failed: ") + dir + "/configuration" + std::to_string(label));
    if (ok) std::copy(c.data(), c.data() + (size_t)rows * cols, config_out);
  });
}
int pepshost_load_configuration(const char *dir, int label, int rows, int cols, int32_t *config_out) {
  return pepshost_load_configuration2(dir, label, rows, cols, config_out, nullptr);
}
// Configuration::StreamRead (configuration.h:446-455) of a text buffer: std::runtime_error (PEPSGPU_EEMPTY) when it holds too few numbers
int pepshost_configuration_from_text(const char *text, int rows, int cols, int32_t *config_out) {
  return guarded([&]() {
    Configuration c(1, rows, cols);
    std::istringstream iss(text);
    StreamReadConfiguration(c, 0, iss);
    std::copy(c.data(), c.data() + (size_t)rows * cols, config_out);
  });
}

// SuwaTodoStateUpdate (suwa_todo_update.h:53-112) alone, on the host: the chain state_{t+1} = SuwaTodoStateUpdate(state_t, weights, gen) of
// n_steps updates with gen = std::mt19937(seed).  No device call: what the reference's test_suwa_todo_update.cpp exercises (single state,
// zero weights, stationary distribution) and the deviate-for-deviate comparison with oracle/vmc.py run on the CPU suite.
int pepshost_suwa_todo_chain(int init_state, const double *weights, int n, uint64_t seed, long n_steps, int32_t *states_out) {
  return guarded([&]() {
    if (n <= 0 || init_state < 0 || init_state >= n) throw std::invalid_argument("pepshost_suwa_todo_chain: init_state outside the weights");
    std::vector<double> w(weights, weights + n);
    for (double x : w)
      if (!(x >= 0.0)) throw std::invalid_argument("pepshost_suwa_todo_chain: negative weight");
    if (!(w[init_state] > 0.0)) throw std::invalid_argument("pepshost_suwa_todo_chain: weights[init_state] must be positive");
    std::mt19937 gen((std::mt19937::result_type)seed);
    size_t state = (size_t)init_state;
    for (long t = 0; t < n_steps; ++t) {
      state = SuwaTodoStateUpdate(state, w, gen);
      states_out[t] = (int32_t)state;
    }
  });
}

}  // extern "C"
