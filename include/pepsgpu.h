/* pepsgpu.h -- C ABI of the MI355X boundary-MPS contraction library (libpepsgpu.so).
 *
 * The reference (QuantumLiquids/PEPS v0.1.0) has NO FFI: its seam is the compile-time
 * `ContractorT` template parameter (include/qlpeps/vmc_basic/wave_function_component.h:136-140,
 * concepts :24-87) filled by `BMPSContractor<TenElemT,QNT>`
 * (include/qlpeps/two_dim_tn/tensor_network_2d/bmps/bmps_contractor.h:187-1027).
 * Each entry point below replaces one method of that class (cited per function), batched over
 * the Monte-Carlo walkers of one GPU: where the reference holds one TensorNetwork2D + one
 * BMPSContractor per MPI rank, a context holds `n` walkers that advance in lockstep.
 *
 * Conventions
 *   - plain pointers and sizes only; host buffers are caller-owned; no exceptions cross the ABI.
 *   - every call returns 0 on success or a PEPSGPU_E* code; pepsgpu_last_error(ctx) gives the text.
 *     The host wrappers re-raise them as the reference's C++ exceptions (bmps_impl.h:839-843,
 *     bmps_contractor.h:221-226, tensor_network_2d_basic_impl.h:37-66).
 *   - positions: LEFT=0, DOWN=1, RIGHT=2, UP=3 (include/qlpeps/basic.h:58-63);
 *     bond orientation: HORIZONTAL=0, VERTICAL=1 (basic.h:19-22).
 *   - site tensors have leg order (L, D, R, U) (tensor_network_2d.h:39-45).
 *   - amplitudes are returned as float64 (the device keeps per-environment log-scales).
 */
#ifndef PEPSGPU_H
#define PEPSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pepsgpu_ctx pepsgpu_ctx;

enum {
  PEPSGPU_OK = 0,
  PEPSGPU_EINVAL = 1,     /* std::invalid_argument */
  PEPSGPU_EHIP = 2,       /* device/runtime failure */
  PEPSGPU_ESTATE = 3,     /* std::logic_error: environment / parameters not ready */
  PEPSGPU_ERANGE = 4,     /* std::out_of_range: configuration value >= physical dim */
  PEPSGPU_EEMPTY = 5,     /* std::runtime_error: empty (zero) tensor, bmps_impl.h:839-843 */
  PEPSGPU_ENOCONV = 6     /* the Jacobi eigensolver of pepsgpu_minsr_direction / pepsgpu_diag_eigh reached its sweep cap */
};
/* element type of the device tensors (TenElemT of the reference: QLTEN_Double, QLTEN_Complex).  PEPSGPU_C128 = complex
 * float64 (std::complex<double> layout, interleaved re / im).  For a complex context EVERY scalar or tensor the calls
 * below return through a `double *` is an interleaved (re, im) pair: out_amp has 2 n doubles, a hole 2 D^4 per walker, a
 * BMPS tensor 2 x elements; pepsgpu_state_upload additionally accepts host_dtype = PEPSGPU_C128.  The complex type covers
 * SVD and (since round 5) variational compression, every contraction / trace / hole entry point, the walker calls, the gradient
 * accumulation (pepsgpu_grad_* below, with the reference's conjugations: psi, eloc and the accumulators are interleaved pairs) and
 * the SR / MinSR family (pepsgpu_sr_*), the device-side sweep slices and the device-side energy slices
 * pepsgpu_nn_exchange_slice_tab / pepsgpu_onsite_slice.  pepsgpu_nn_exchange_slice alone is real only and returns
 * PEPSGPU_EINVAL on a complex context. */
enum { PEPSGPU_F32 = 0, PEPSGPU_F64 = 1, PEPSGPU_C128 = 3 };
enum { PEPSGPU_LEFT = 0, PEPSGPU_DOWN = 1, PEPSGPU_RIGHT = 2, PEPSGPU_UP = 3 };
enum { PEPSGPU_HORIZONTAL = 0, PEPSGPU_VERTICAL = 1 };
enum { PEPSGPU_SVD_COMPRESS = 0, PEPSGPU_VARIATION2SITE = 1, PEPSGPU_VARIATION1SITE = 2 };   /* CompressMPSScheme, bmps.h:31-35 */

/* BMPSContractor(rows, cols) + SetTruncateParams(BMPSTruncateParams{D_min, D_max, trunc_err, scheme})
 * (bmps_contractor.h:187-226, bmps.h:47-98).  dtype = element type of the device tensors. */
int pepsgpu_ctx_create(pepsgpu_ctx **out, int device, int dtype, int rows, int cols, int D, int phys_dim,
                       int chi_min, int chi_max, double trunc_err, int scheme, int max_walkers);
/* BMPSContractor::SetTruncateParams (bmps_contractor.h:216) with the full BMPSTruncateParams (bmps.h:47-98):
 * D_min, D_max, trunc_err, scheme and, for the variational schemes, convergence_tol and iter_max
 * (BMPS::MultiplyMPO2SiteVariationalCompress_ / 1Site, bmps_impl.h:864-1172; bosonic only as in the reference).
 * Takes effect at the next absorption; existing BMPS stacks are kept.  A context created with a variational scheme
 * uses convergence_tol = 1e-10, iter_max = 10 until this is called. */
int pepsgpu_set_truncate_params(pepsgpu_ctx *ctx, int chi_min, int chi_max, double trunc_err, int scheme,
                                double convergence_tol, int iter_max);
void pepsgpu_ctx_destroy(pepsgpu_ctx *ctx);
const char *pepsgpu_last_error(pepsgpu_ctx *ctx);

/* SplitIndexTPS (two_dim_tn/tps/split_index_tps.h:80-606) as one flat host buffer
 * [row][col][s][L][D][R][U], every leg zero-padded to D; host_dtype = PEPSGPU_F32 / PEPSGPU_F64.
 * Replaces the MPI_Bcast of the state (mc_energy_grad_evaluator.h:161). */
int pepsgpu_state_upload(pepsgpu_ctx *ctx, const void *sitps_flat, int host_dtype);

/* TensorNetwork2D(sitps, config) + BMPSContractor::Init(tn) for n walkers
 * (tensor_network_2d_basic_impl.h:24-74, bmps_contractor_init.h:25-70).  configs = [n][rows][cols]. */
int pepsgpu_walkers_set_configs(pepsgpu_ctx *ctx, int n, const int32_t *configs);
int pepsgpu_walkers_get_configs(pepsgpu_ctx *ctx, int32_t *configs_out);
int pepsgpu_n_walkers(pepsgpu_ctx *ctx);

/* BMPS stacks -- bmps_contractor_grow.h */
int pepsgpu_grow_bmps_step(pepsgpu_ctx *ctx, int pos);          /* GrowBMPSStep(tn,pos)      :32-47   */
int pepsgpu_grow_full_bmps(pepsgpu_ctx *ctx, int pos);          /* GrowFullBMPS              :49-86   */
int pepsgpu_grow_bmps_for_row(pepsgpu_ctx *ctx, int row);       /* GrowBMPSForRow            :88-104  */
int pepsgpu_grow_bmps_for_col(pepsgpu_ctx *ctx, int col);       /* GrowBMPSForCol            :106-122 */
int pepsgpu_shift_bmps_window(pepsgpu_ctx *ctx, int pos);       /* ShiftBMPSWindow           :143-148 */
int pepsgpu_delete_inner_bmps(pepsgpu_ctx *ctx, int pos);       /* DeleteInnerBMPS  bmps_contractor.h:320-324 */
/* BMPSWalker (bmps/impl/bmps_walker.h:  a BMPS forked out of a stack, evolved row by row and contracted against an
 * explicitly named environment of the opposite stack).  The stack itself is the walker here: park hides the levels
 * above keep_levels (no copy) so that the BTen / trace calls see level keep_levels-1 as the top; unpark drops what was
 * grown meanwhile and restores the hidden levels. */
int pepsgpu_bmps_park(pepsgpu_ctx *ctx, int pos, int keep_levels);
int pepsgpu_bmps_unpark(pepsgpu_ctx *ctx, int pos);
/* One row (orientation = PEPSGPU_HORIZONTAL, slice = row) or column (PEPSGPU_VERTICAL, slice = column) of the Monte-Carlo sweep with
 * the nearest-neighbour EXCHANGE updater, entirely on the device: replaces, for that slice, the loop body of
 * MCUpdateSquareNNUpdateBaseOBC::operator() (square_nn_updater.h:41-55 / :62-76: InitBTen, GrowFullBTen(.., 2, true), then per bond
 * TwoSiteNNUpdateLocalImpl + ShiftBTenWindow) with MCUpdateSquareNNExchangeOBC::TwoSiteNNUpdateLocalImpl (:142-189: skip equal
 * spins, ReplaceNNSiteTrace of the exchanged pair, Metropolis on |psi'/psi|^2, UpdateLocal).  The BMPS pair of the slice must be in
 * place as for pepsgpu_init_bten (the caller keeps doing GenerateBMPSApproach / ShiftBMPSWindow between slices).
 *   uniforms        [n][n_uniform], n_uniform >= slice length - 1: per walker the NEXT deviates of its std::mt19937 +
 *                   uniform_real_distribution<double>(0, 1) stream, in drawing order; a walker consumes one only where the
 *                   reference draws one (spins differ and |psi'| < |psi|), consumed_out[w] says how many -- the chain is the
 *                   reference's chain when the caller pops exactly those from its queue;
 *   amplitude_inout [n] psi of every walker before / after the slice;  accepted_out [n] accepted exchanges;
 *   slice_states_out [n][slice length] (may be NULL) the configuration along the slice after the pass.
 * Every element type (round 6; a PEPSGPU_C128 context takes and returns interleaved (re, im) amplitudes, the test is on |psi'| / |psi|). */
int pepsgpu_sweep_slice_exchange(pepsgpu_ctx *ctx, int orientation, int slice, int n_uniform, const double *uniforms,
                                 double *amplitude_inout, int32_t *consumed_out, int32_t *accepted_out, int32_t *slice_states_out);
/* The same with the move given as a table (round 6): pair_table [phys_dim^2][2] (phys_dim = that of the context), the pair of states the
 * "exchange" proposes for the states (a, b) of a bond = pair_table[a * phys_dim + b]; NULL = the swap (b, a).  A fermionic state lives on
 * the device as EXTENDED states (state + d * variant: mode order x parity of the fermions before the site); the exchange of two sites
 * adjacent in the mode order changes their variants by a rule local in (a, b) -- TPSWaveFunctionComponent::DeviceStatesNN
 * (peps_amd/host/qlpeps_gpu.h) tabulated -- so MCUpdateSquareNNExchangeOBC on a fermionic state runs on the device too
 * (square_nn_updater.h:142-189 with the fermionic UpdateLocal of wave_function_component.h:345-378).  The amplitudes are those of
 * the decorated network of the current mode order (no sign factors: the Metropolis test sees moduli only; the caller restores
 * Sigma / Kappa from the configuration it gets back). */
int pepsgpu_sweep_slice_exchange_tab(pepsgpu_ctx *ctx, int orientation, int slice, int n_uniform, const double *uniforms,
                                     const int32_t *pair_table, double *amplitude_inout, int32_t *consumed_out, int32_t *accepted_out,
                                     int32_t *slice_states_out);
/* One row / column of MCUpdateSquareNNFullSpaceUpdateOBC (square_nn_updater.h:253-293) on the device: per bond the replacement trace of
 * all phys_dim^2 states of the pair (ReplaceNNSiteTrace with phys_dim^2 candidates), the weights |psi_k / psi|^2 (the current state
 * keeps its stored amplitude), SuwaTodoStateUpdate (suwa_todo_update.h:53-112) and UpdateLocal.
 *   engine_words [n][2 (slice length - 1)]: per walker the next raw 32-bit outputs of its std::mt19937 -- the reference draws
 *                std::uniform_real_distribution<long double>, i.e. two words per bond whatever the data, so the walker's engine is
 *                consumed exactly as by the reference's updater (identical chains; the kernel's arithmetic is float64 where
 *                SuwaTodoStateUpdate uses long double: a decision can differ only within 2^-53 of a boundary of the cumulative weights);
 *   phys_dim     states per site the move ranges over (phys_dim^2 <= 16); bosonic states (not the extended fermionic ones);
 *   amplitude_inout, accepted_out, slice_states_out as above (accepted = moves that changed the pair). */
int pepsgpu_sweep_slice_fullspace(pepsgpu_ctx *ctx, int orientation, int slice, int phys_dim, const uint32_t *engine_words,
                                  double *amplitude_inout, int32_t *accepted_out, int32_t *slice_states_out);
/* One row / column of MCUpdateSquareTNN3SiteExchange on the device (MCUpdateSquareTNN3SiteUpdateBase::operator(),
 * square_3site_updater.h:36-56 row pass, :61-81 column pass; TNN3SiteUpdateImpl :109-158): InitBTen + GrowFullBTen(.., 3, true), the
 * amplitude reset to the ReplaceTNNSiteTrace of the first window (:39-42, :64-67), then per triple of consecutive sites its distinct
 * permutations as candidates (ReplaceTNNSiteTrace; a triple of three equal states does no trace and draws nothing, :118), the weights
 * norm(psi_i / max |psi|) with the stored amplitude at the current triple, SuwaTodoStateUpdate, UpdateLocal and ShiftBTenWindow.
 *   triple_table [phys_dim^3][20] (phys_dim = that of the context), indexed by e1 phys_dim^2 + e2 phys_dim + e3: m (1, 3 or 6 distinct
 *                permutations), init (the slot of the triple itself), six slots of three states in std::next_permutation order of the
 *                sorted triple, unused slots repeating slot 0; NULL = the bosonic table of the context's phys_dim.  Fermions: the
 *                permutations of the physical triple as extended states (the three sites are consecutive modes of the current order);
 *                phys_dim == 2 takes 3 candidate slots per triple, every other phys_dim 6;
 *   engine_words [n][n_words], n_words >= 2 (slice length - 2): the next raw 32-bit outputs of each walker's std::mt19937 (the long double
 *                draw of SuwaTodoStateUpdate = two words); consumed_out [n] how many walker w took (0 or 2 per triple);
 *   amplitude_out [n] the amplitude after the slice (interleaved (re, im) for PEPSGPU_C128; fermions: of the decorated network, the
 *                caller restores Sigma / Kappa); not read on entry -- the slice resets it;
 *   accepted_out [n] moves that changed the triple; slice_states_out [n][slice length] (may be NULL) as above.
 * Status 1: bad orientation or slice, a lattice with fewer than 3 rows or columns, n_words < 2 (slice length - 2); 4: a table entry out
 * of range.  Either leaves the configuration untouched. */
int pepsgpu_sweep_slice_tnn3(pepsgpu_ctx *ctx, int orientation, int slice, const int32_t *triple_table, int n_words,
                             const uint32_t *engine_words, double *amplitude_out, int32_t *consumed_out, int32_t *accepted_out,
                             int32_t *slice_states_out);
/* The bosonic triple table pepsgpu_sweep_slice_tnn3 builds when it is given none: out [phys_dim^3][20], 1 <= phys_dim <= 64 (else
 * PEPSGPU_EINVAL).  Host only: needs no context and no device. */
int pepsgpu_diag_tnn3_table(int phys_dim, int32_t *out);

/* One row / column of the energy evaluation for models whose nearest-neighbour off-diagonal term exchanges the two site states (XXZ,
 * J1-J2, t-J ...): the slice part of SquareNNNModelEnergySolver::CalEnergyAndHolesImpl (square_nnn_energy_solver.h:142-200 row pass:
 * InitBTen, GrowFullBTen(RIGHT, row, 1, true), psi = Trace, per site PunchHole, per bond the ReplaceNNSiteTrace of the exchanged pair
 * + ShiftBTenWindow) and of the column pass (bond_traversal_mixin.h:120-144: GrowFullBTen(DOWN, col, 2, true), no holes) on the device
 * with ONE read-back: psi_out [n], psi_exchanged_out [n][slice length - 1] (amplitude of the configuration with the two sites of bond
 * j exchanged; for equal states it is psi).  punch_holes != 0: the holes of the slice's sites are stored in HBM as pepsgpu_punch_hole
 * with out == NULL does.  The BMPS pair of the slice must be in place.  Real element types only. */
int pepsgpu_nn_exchange_slice(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, double *psi_out, double *psi_exchanged_out);
/* The exchange slice of every element type (a PEPSGPU_C128 context returns interleaved (re, im) amplitudes), with the move as a table
 * and, for the fermionic models, psi per bond.  Replaces the per-bond hooks of SquareNNNModelEnergySolver (square_nnn_energy_solver.h:
 * 142-200, bond_traversal_mixin.h:120-144) for complex states and for the fermionic EvaluateBondEnergy (square_spinless_fermion.h:
 * 134-159, square_tJ_model.h:301-345: Trace + ReplaceNNSiteTrace per bond).
 *   pair_table    [phys_dim^2][2] as for pepsgpu_sweep_slice_exchange_tab (fermions: the exchange of two extended states adjacent in
 *                 the current mode order); NULL = the swap (b, a).  A table entry outside [0, phys_dim) is PEPSGPU_ERANGE;
 *   psi_per_bond  0: psi_out [n], the Trace of the slice's first window (as pepsgpu_nn_exchange_slice);
 *                 != 0: psi_out [n][slice length - 1], per bond the Trace of the window before that bond's replacement trace;
 *   psi_exchanged_out [n][slice length - 1] the amplitude with the move of bond j applied (psi of bond j where it is the identity).
 * With a NULL table and psi_per_bond = 0 a real context returns exactly what pepsgpu_nn_exchange_slice returns. */
int pepsgpu_nn_exchange_slice_tab(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, const int32_t *pair_table,
                                  int psi_per_bond, double *psi_out, double *psi_exchanged_out);
/* One row / column of one-site moves on the device, every element type: TransverseFieldIsingSquareOBC's row pass
 * (transverse_field_ising_square_obc.h:195-203: InitBTen, GrowFullBTen(.., 1, true), psi = Trace, per site PunchHole and
 * ReplaceOneSiteTrace of the flipped state, ShiftBTenWindow) with SquareNNNModelEnergySolver's PunchHole, ONE read-back.
 *   site_table   [phys_dim][n_cand]: candidate k of a site in state s is site_table[s * n_cand + k] (TFIM: {1, 0}, n_cand = 1);
 *                an entry outside [0, phys_dim) is PEPSGPU_ERANGE, n_cand < 1 PEPSGPU_EINVAL;
 *   psi_out [n]; psi_cand_out [n][slice length][n_cand] the amplitude with site j of the slice in candidate state k;
 *   punch_holes != 0: the holes of the slice's sites are stored in HBM as pepsgpu_punch_hole with out == NULL does.
 * The BMPS pair of the slice must be in place; the BTen stacks are left as the per-site calls leave them. */
int pepsgpu_onsite_slice(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, int n_cand, const int32_t *site_table,
                         double *psi_out, double *psi_cand_out);
/* The next-nearest-neighbour (diagonal) bonds of the row pair (row1, row1 + 1) on the device, every element type: the NNN block of
 * SquareNNNModelEnergySolver::CalEnergyAndHolesImpl (square_nnn_energy_solver.h:203-265: InitBTen2(LEFT, row1), GrowFullBTen2(RIGHT,
 * row1, 2, true), then per column the ReplaceNNNSiteTrace of each diagonal with its two end states exchanged and ShiftBTen2Window(RIGHT,
 * row1), after the last column too) with ONE read-back.  Preconditions of the row pass: the UP boundary MPS at row1 and the DOWN one at
 * row1 + 1, i.e. the state after that row's nearest-neighbour slice and before ShiftBMPSWindow(DOWN).
 *   diag_mask  bit 0: LEFTUP_TO_RIGHTDOWN, (row1, c) <-> (row1 + 1, c + 1); bit 1: LEFTDOWN_TO_RIGHTUP, (row1 + 1, c) <-> (row1, c + 1);
 *   val_out    [n][cols - 1][2] (PEPSGPU_C128: interleaved (re, im)): the amplitude of the configuration with the two ends of diagonal
 *              `kind` of plaquette c exchanged; 0.0 for a diagonal that is not in the mask and for equal end states (the identity: the
 *              reference contracts nothing there, square_spin_onehalf_xxz_obc.h:107-134; the caller decides it from the configuration).
 * The BTen2 stacks end as the per-plaquette calls leave them.  Status PEPSGPU_EINVAL: row1 outside [0, rows - 2], diag_mask outside 1..3,
 * a NULL buffer; PEPSGPU_ESTATE: a boundary MPS of the row pair is missing, or a configuration override (pepsgpu_cfg_override_slice) is
 * active -- the slice reads the walkers' own configuration table, i.e. it serves bosonic configurations of every element type; the
 * fermionic diagonal hop has its own slice, pepsgpu_nnn_hop_slice_fermion.  A refused call leaves the context usable. */
int pepsgpu_nnn_exchange_slice(pepsgpu_ctx *ctx, int row1, int diag_mask, double *val_out);
/* Completed pepsgpu_nnn_exchange_slice calls of this process (all contexts): lets a caller prove which path computed its numbers. */
long pepsgpu_diag_nnn_slice_calls(void);
/* The diagonal hops of the row pair (row1, row1 + 1) of a FERMIONIC state on the device, every element type (square_spinless_fermion.h:
 * 161-200, square_tJ_model.h:424-463).  The walkers' configurations are extended states e = s + d * variant in row-major order (variant
 * 0 / 1), the context's physical dimension is 4 d; occ [d] (0 / 1) is the fermion number of each physical state.  A hop along a diagonal
 * exchanges the physical states of its two ends and flips the variant of every site between them in row-major order, so the hopped
 * amplitude is a replacement of the four plaquette tensors against twisted environments.  In order: BTen2 set 0 gets GrowFullBTen2(RIGHT,
 * row1, 2, true) and InitBTen2(LEFT, row1); set 1 gets the RIGHT chain grown with row row1 variant-flipped and the LEFT chain with row
 * row1 + 1 variant-flipped; per plaquette psi comes from the walkers' own four states between the set-0 environments and the hopped
 * amplitude of each requested diagonal from the hopped states between the set-1 environments; then both LEFT chains advance one column.
 * ONE read-back, no upload: the flipped tables, the candidates and the signs are built on the device.
 *   diag_mask  as for pepsgpu_nnn_exchange_slice;
 *   psi_out    [n][cols - 1] (PEPSGPU_C128: interleaved (re, im)): psi of plaquette c along the same contraction path; 0.0 for a plaquette
 *              where no walker has an allowed hop on a requested diagonal (it only advances the chains);
 *   val_out    [n][cols - 1][2]: jw * psi' of diagonal `kind` of plaquette c, jw = (-1)^(fermions strictly between the two ends in row-major
 *              order) already applied; 0.0 for a diagonal outside the mask and for a forbidden hop, occ[state_a] == occ[state_b].
 * On return, and after any error, BTen2 set 0 is selected and no configuration override is active; the BMPS stacks are untouched.
 * Status PEPSGPU_EINVAL: row1 outside [0, rows - 2], diag_mask outside 1..3, a NULL buffer, 4 * d != the context's physical dimension, an
 * occ entry outside {0, 1}; PEPSGPU_ESTATE: a boundary MPS of the row pair is missing, a configuration override or BTen2 set 1 is
 * active on entry, or a state of variant >= 2 (a column-major table) in either row.  A refused call leaves the context usable. */
int pepsgpu_nnn_hop_slice_fermion(pepsgpu_ctx *ctx, int row1, int d, const int32_t *occ, int diag_mask, double *psi_out, double *val_out);
/* Completed pepsgpu_nnn_hop_slice_fermion calls of this process (all contexts). */
long pepsgpu_diag_nnn_hop_slice_calls(void);
/* The candidate kernel of pepsgpu_nnn_hop_slice_fermion alone, on the caller's extended configurations ext [n][rows][cols] (states in
 * [0, 2 d)) for the plaquette (row1, col1): cand_out [n][2][4] the hopped extended states of (row1, col1), (row1 + 1, col1),
 * (row1 + 1, col1 + 1), (row1, col1 + 1) for LEFTUP_TO_RIGHTDOWN and LEFTDOWN_TO_RIGHTUP; sign_out [n][2] = +1 / -1, 0 for a forbidden
 * hop; flag_out [n][2] = -1 where the hop is allowed, else 1 (the skip-flag convention of the slice).  Needs a device, no context. */
int pepsgpu_diag_fermion_hop_cand(int rows, int cols, int d, const int32_t *occ, int n, const int32_t *ext, int row1, int col1,
                                  int32_t *cand_out, int32_t *sign_out, int32_t *flag_out);
/* One row (PEPSGPU_HORIZONTAL) or column (PEPSGPU_VERTICAL) of a FERMIONIC state for the measurement of pair operators on its
 * nearest-neighbour bonds next to the bond energy (square_tJ_model.h:301-345 EvaluateBondEnergy, :546-603 EvaluateBondSC), every element
 * type, ONE read-back and no per-bond upload.  The walkers' configurations are extended states e = s + d * variant of the mode order of
 * the pass (row pass: row-major, variants 0 / 1; column pass: column-major, variants 2 / 3), the context's physical dimension is 4 d;
 * occ [d] (0 / 1) is the fermion number of each physical state.  In order: InitBTen, GrowFullBTen(.., 2, true), then per bond j the Trace
 * of the window, ONE ReplaceNNSiteTrace over the exchange candidate and the two pair candidates, and ShiftBTenWindow while j + 2 < slice
 * length -- the BTen stacks end as the per-bond calls leave them.
 *   pair_table      [d * d][2][2] over PHYSICAL states: candidate k of the states (a, b) on (left / upper, right / lower) site is
 *                   (a'_k, b'_k) = pair_table[((a * d + b) * 2 + k) * 2 ..], (-1, -1) for none.  A candidate keeps the fermion parity of
 *                   the pair, so only the variants of the two sites change; the device derives them from occ;
 *   exchange_table  [phys_dim^2][2] over extended states as for pepsgpu_nn_exchange_slice_tab, or NULL: no exchange candidate, ex_out is
 *                   not written;
 *   psi_out   [n][slice length - 1] (PEPSGPU_C128: interleaved (re, im), as every output here): the Trace before bond j's replacement;
 *   ex_out    [n][slice length - 1]: the amplitude with the exchange move of bond j applied (psi of bond j where it is the identity);
 *   pair_out  [n][slice length - 1][2]: sign * psi' of pair candidate k of bond j, sign = Sigma(S') / Sigma(S) of the decoration
 *             Sigma = (-1)^(nf (nf + 1) / 2): -1 where the candidate changes the fermion number by +-2, +1 where it keeps it; exactly 0.0
 *             for "no candidate".  pair_out / psi_out is the ratio of the graded amplitudes times the Jordan-Wigner sign of the sites
 *             strictly between the two in row-major order (+1 for a bond along a row).
 * Status PEPSGPU_EINVAL: bad orientation or slice, a NULL required buffer (ex_out is required with an exchange_table), 4 * d != the
 * context's physical dimension, an occ entry outside {0, 1}, a pair_table entry outside [-1, d), a candidate with only one -1 or one
 * that changes the fermion parity of the pair; PEPSGPU_ERANGE: an exchange_table entry outside [0, phys_dim); PEPSGPU_ESTATE: a
 * boundary MPS of the slice is missing, a configuration override is active, or a state of the slice has a variant of the other mode
 * order.  A refused call leaves the context usable. */
int pepsgpu_nn_pair_slice_fermion(pepsgpu_ctx *ctx, int orientation, int slice, int d, const int32_t *occ, const int32_t *pair_table,
                                  const int32_t *exchange_table, double *psi_out, double *ex_out, double *pair_out);
/* Completed pepsgpu_nn_pair_slice_fermion calls of this process (all contexts). */
long pepsgpu_diag_pair_slice_calls(void);
/* The candidate kernel of pepsgpu_nn_pair_slice_fermion alone, on the caller's extended configurations ext [n][rows][cols] (states in
 * [0, 4 d), of the mode order of `orientation` on the two sites) for the bond (site1, site2): flat row-major indices of the left / upper
 * and the right / lower site.  cand_out [n][2][2] the extended states of the two sites under candidate k (the walker's own two states
 * where it has none); sign_out [n][2] = +1 / -1 as above, 0 for "no candidate".  Needs a device, no context. */
int pepsgpu_diag_pair_cand(int rows, int cols, int d, const int32_t *occ, const int32_t *pair_table, int n, const int32_t *ext,
                           int orientation, int site1, int site2, int32_t *cand_out, int32_t *sign_out);
/* One row / column of a FERMIONIC state for a model whose bond term is up to two hops, the Hubbard model (square_hubbard_model.h:190-262
 * EvaluateBondEnergy: Trace + ReplaceNNSiteTrace of the hopped pairs, nothing for equal states :200-202): pepsgpu_nn_pair_slice_fermion
 * without the exchange slot and, with punch_holes != 0, as the row pass of the energy evaluation (square_nn_energy_solver.h: InitBTen,
 * GrowFullBTen(.., 1, true), per site PunchHole into HBM as pepsgpu_punch_hole with out == NULL does, before that site's bond, and
 * ShiftBTenWindow after every bond, the last one too).  punch_holes == 0 returns the bytes of pepsgpu_nn_pair_slice_fermion with a
 * NULL exchange_table.
 *   hop_table  [d * d][2][2] over PHYSICAL states, the layout and the rules of pair_table above: slot 0 the pair with the up electron
 *              hopped across the bond, slot 1 with the down electron hopped, (-1, -1) where there is no such hop;
 *   psi_out    [n][slice length - 1]; hop_out [n][slice length - 1][2] = sign * psi' as pair_out above: sign = -1 where the
 *              hop changes the number of odd sites by +-2, (up-down, empty) <-> (up, down).
 * Status codes as for pepsgpu_nn_pair_slice_fermion.  A refused call leaves the context usable. */
int pepsgpu_nn_hop_slice_fermion(pepsgpu_ctx *ctx, int orientation, int slice, int punch_holes, int d, const int32_t *occ,
                                 const int32_t *hop_table, double *psi_out, double *hop_out);
/* Completed pepsgpu_nn_hop_slice_fermion calls of this process (all contexts). */
long pepsgpu_diag_hop_slice_calls(void);
/* One row / column of MCUpdateSquareNNUpdateBaseOBC::operator() (square_nn_updater.h:41-55 / :62-76: InitBTen, GrowFullBTen(.., 2, true),
 * per bond TwoSiteNNUpdateLocalImpl + ShiftBTenWindow while j + 2 < slice length) with the move of MCUpdateSquareNNHubbardU1U1OBC
 * (square_hubbard_u1u1_updater.h:95-157) on the device, every element type: per bond the candidates of the pair's sector from a table,
 * ONE ReplaceNNSiteTrace over max_cand slots, the weights |psi_k / psi|^2 (the current state keeps its stored amplitude, :129),
 * SuwaTodoStateUpdate (suwa_todo_update.h:53-112) and UpdateLocal.
 *   sector_table [d * d][2 + 2 max_cand] over PHYSICAL states, 1 <= max_cand <= 16: row a * d + b of the states (a, b) on the (left / upper,
 *                right / lower) site holds m (the size of the sector), init (the slot of (a, b) itself) and max_cand slots (a'_k, b'_k) in
 *                the order of EnumerateHubbardTwoSiteConfigsWithU1U1 (:57-72; Suwa-Todo depends on it); slots m .. max_cand - 1 are (-1, -1);
 *   occ          [d] (0 / 1), the fermion number of each physical state: a fermionic context of physical dimension 4 d whose walkers hold
 *                extended states of the mode order of the pass (as for pepsgpu_nn_pair_slice_fermion); every candidate must keep the
 *                fermion parity of the pair, the device derives the two variants.  NULL: a bosonic context of physical dimension d;
 *   engine_words [n][n_words], n_words >= 2 (slice length - 1): the next raw 32-bit outputs of each walker's std::mt19937; a bond with m <= 1
 *                draws nothing (:114-116), one with m > 1 takes the walker's next two words; consumed_out [n] how many walker w took;
 *   amplitude_inout [n] psi before / after the slice (PEPSGPU_C128: interleaved; fermions: of the decorated network, as for
 *                pepsgpu_sweep_slice_exchange_tab); accepted_out [n] moves that changed the pair; slice_states_out [n][slice length] or NULL.
 * Status PEPSGPU_EINVAL: bad orientation or slice, a NULL required buffer, n_words < 2 (slice length - 1), max_cand outside [1, 16], a
 * physical dimension that is not 4 d (d with a NULL occ), an occ entry outside {0, 1}, a table row with m outside [1, max_cand], init
 * outside [0, m), a -1 in a used slot, a state in an unused one, a slot init that is not (a, b), or a candidate that changes the fermion
 * parity; PEPSGPU_ERANGE: a table state outside [-1, d); PEPSGPU_ESTATE: a boundary MPS of the slice is missing, a configuration override is
 * active, or a state of the slice has a variant of the other mode order.  A refused call leaves the configuration untouched and the
 * context usable. */
int pepsgpu_sweep_slice_sector(pepsgpu_ctx *ctx, int orientation, int slice, int d, const int32_t *occ, int max_cand,
                               const int32_t *sector_table, int n_words, const uint32_t *engine_words, double *amplitude_inout,
                               int32_t *consumed_out, int32_t *accepted_out, int32_t *slice_states_out);
/* Completed pepsgpu_sweep_slice_sector calls of this process (all contexts). */
long pepsgpu_diag_sector_slice_calls(void);
/* The candidate kernel of pepsgpu_sweep_slice_sector alone, on the caller's configurations ext [n][rows][cols] (occ given: extended
 * states in [0, 4 d) of the mode order of `orientation` on the two sites; occ NULL: states in [0, d)) for the bond (site1, site2), flat
 * row-major indices.  cand_out [n][max_cand][2] the states of the two sites in slot k (the walker's own two states in an unused slot);
 * meta_out [n][2] = (m, init).  Needs a device, no context. */
int pepsgpu_diag_sector_cand(int rows, int cols, int d, const int32_t *occ, int max_cand, const int32_t *sector_table, int n,
                             const int32_t *ext, int orientation, int site1, int site2, int32_t *cand_out, int32_t *meta_out);
/* The links of a row pair or a column pair on the device, every element type: the bodies of the row-pair loop and of the column-pair
 * loop of the triangular J1-J2 model (spin_onehalf_triangle_heisenbergJ1J2_sqrpeps.h:350-398, :425-442) with ONE read-back and no
 * upload.  (r, c) is the upper-left site of the window; bit k of link_mask requests kind k:
 *   PEPSGPU_HORIZONTAL (slice1 = row r, rows r, r + 1; N = cols)
 *     0  diagonal (r, c)-(r + 1, c + 1)                   1  diagonal (r + 1, c)-(r, c + 1)
 *     2  flat link (r, c)-(r + 1, c + 2)                  3  flat link (r + 1, c)-(r, c + 2)
 *     InitBTen2(LEFT, r), GrowFullBTen2(RIGHT, r, 2, true), then per column ReplaceNNNSiteTrace of each requested diagonal,
 *     ReplaceSqrt5DistTwoSiteTrace of each requested flat link and ShiftBTen2Window(RIGHT, r), after the last column too.  Needs the UP
 *     boundary MPS at r and the DOWN one at r + 1.
 *   PEPSGPU_VERTICAL (slice1 = column c, columns c, c + 1; N = rows >= 3)
 *     2  steep link (r, c)-(r + 2, c + 1)                 3  steep link (r + 2, c)-(r, c + 1)
 *     InitBTen2(UP, c), GrowFullBTen2(DOWN, c, 3, true), then per row the ReplaceSqrt5DistTwoSiteTrace of each requested steep link and
 *     ShiftBTen2Window(DOWN, c) while r + 3 < rows.  Needs the LEFT boundary MPS at c and the RIGHT one at c + 1.
 *   val_out  [n][N - 1][4] (PEPSGPU_C128: interleaved (re, im)): the amplitude of the configuration with the two end states of link
 *            `kind` of window position j exchanged; exactly 0.0 for a kind that is not in the mask, for equal end states (the identity:
 *            the caller decides it from the configuration) and for a position without such a link (the last column / row).
 * The BTen2 stacks end as the per-call sequence leaves them.  Status PEPSGPU_EINVAL: a bad orientation, slice1 outside the lattice,
 * link_mask outside 1..15, bit 0 or 1 in a vertical call, a vertical call on fewer than three rows, a NULL buffer; PEPSGPU_ESTATE: a
 * boundary MPS of the pair is missing, or a configuration override is active (bosonic configurations only, as
 * pepsgpu_nnn_exchange_slice).  A refused call leaves the context usable. */
int pepsgpu_link_exchange_slice(pepsgpu_ctx *ctx, int orient, int slice1, int link_mask, double *val_out);
/* Completed pepsgpu_link_exchange_slice calls of this process (all contexts); pepsgpu_diag_nnn_slice_calls does not count them. */
long pepsgpu_diag_link_slice_calls(void);
/* The candidate kernel of the sqrt5 links of pepsgpu_link_exchange_slice alone, on the caller's configurations cfg [n][rows][cols]
 * (states in [0, phys_dim)) for the window at (row1, col1): 2 x 3 for PEPSGPU_HORIZONTAL, 3 x 2 for PEPSGPU_VERTICAL.  cand_out
 * [n][2][4]: the states of the window's corners (upper-left, lower-left, lower-right, upper-right) with the ends of link kind 2, then of
 * kind 3, exchanged; flag_out [n][2] = -1 where the end states differ, else 1 (the skip-flag convention of the slice).  Needs a device,
 * no context. */
int pepsgpu_diag_link_cand(int rows, int cols, int phys_dim, int n, const int32_t *cfg, int orient, int row1, int col1, int32_t *cand_out,
                           int32_t *flag_out);

/* BMPSWalker as an object -- BMPSContractor::GetWalker / class BMPSWalker, bmps_contractor.h:357-646, bmps/impl/bmps_walker.h:13-465.
 * A walker holds the fork of the top BMPS of stack `pos` for every Monte-Carlo walker of the context (deep copy; the stacks are not
 * touched afterwards), its stack-size counter and its own LEFT / RIGHT BTen caches.  The TransferMPO the calls below absorb / sandwich
 * is named once with pepsgpu_walker_set_mpo: slice `num` of the network (a row for UP / DOWN walkers, a column for LEFT / RIGHT)
 *   states == NULL && tensors == NULL : under the walkers' current configurations,
 *   states  [n][N] (N = slice length)  : with the given SITPS component at every site of the slice, per walker (an excited row),
 *   tensors [n_tensors][N][D^4]        : explicit site tensors, float64 (interleaved pairs for PEPSGPU_C128), leg order (L, D, R, U)
 *                                        zero padded to D, leg dims of the slice's sites; n_tensors = 1 (shared) or n -- an MPO that is
 *                                        NOT a row of the context's network (Evolve(const TransferMPO &), bmps_walker.h:13-21).
 * The opposite boundary of the row operations is level `opp_level` of the DOWN stack (down_stack[opp_level] of the reference's tests:
 * the boundary that has absorbed opp_level rows from below); only the UP walker / DOWN opposite pair is supported, as in the reference
 * (bmps_walker.h:114-118: anything else -> PEPSGPU_EINVAL).  Errors of the reference's runtime_error checks -> PEPSGPU_ESTATE.
 * A walker dies with pepsgpu_walkers_set_configs (it is a fork of the old configurations' stacks). */
/* level < 0: GetWalker(tn, pos) :51-58 (fork of the top of the stack); level >= 0: BMPSWalker(tn, stack[level], pos, level + 1,
 * trunc_params), the constructor the structure-factor mixin uses on the vacuum (structure_factor_measurement_mixin.h:121-122) */
int pepsgpu_walker_create(pepsgpu_ctx *ctx, int pos, int level, int *walker_out);
/* copy construction (`auto excited_walker = main_walker;`, :134); the BTen caches of the copy start empty */
int pepsgpu_walker_clone(pepsgpu_ctx *ctx, int walker, int *walker_out);
int pepsgpu_walker_destroy(pepsgpu_ctx *ctx, int walker);
/* GetPosition / GetStackSize / GetBTenLeftCol / GetBTenRightCol (any pointer may be NULL) */
int pepsgpu_walker_info(pepsgpu_ctx *ctx, int walker, int *pos_out, int *stack_size_out, int *bten_left_col_out, int *bten_right_col_out);
int pepsgpu_walker_set_mpo(pepsgpu_ctx *ctx, int walker, int num, const int32_t *states, const double *tensors, int n_tensors);
/* The excited row of the structure-factor measurement (structure_factor_measurement_mixin.h:62-215: the MPO of row y1 with the tensor
 * of the source site replaced, :127-134) without a host table: the walker's MPO becomes slice `num` under the walkers' current
 * configurations with the state s of site `col` of that slice replaced, per walker, by state_map[s] (state_map has phys_dim entries,
 * phys_dim <= 32).  The table the kernels read is built on the device -- a device-to-device copy of the configuration table and a
 * one-site patch kernel -- with no upload and no synchronisation; open_out [n] (may be NULL) = 1 where state_map[s] != s, from the
 * host's mirror of the configurations.  Afterwards the walker is exactly as after pepsgpu_walker_set_mpo(.., states, ..) with that row.
 * UP walkers only.  Status PEPSGPU_EINVAL: NULL state_map, num or col outside the lattice, a walker that is not UP; PEPSGPU_ERANGE: a
 * map entry outside [0, phys_dim).  A refused call leaves the walker and its MPO as they were. */
int pepsgpu_walker_set_mpo_excited(pepsgpu_ctx *ctx, int walker, int num, int col, const int32_t *state_map, uint8_t *open_out);
/* The scan of one target row (structure_factor_measurement_mixin.h:160-194 on bmps_walker.h:216-392) in one call with one read-back, for
 * the walker's current MPO when that is a row named by configuration or by states (N = cols):
 *   InitBTenLeft(opp, N), InitBTenRight(opp, N - 1), then for x2 = N - 1 .. 0: TraceWithBTen at x2 with the site's state s replaced by
 *   site_map[s] (phys_dim entries), and GrowBTenRightStep while x2 > 0.
 *   out [n][N] (PEPSGPU_C128: interleaved (re, im)): entry (w, x2) is that trace where walker_mask[w] != 0 (NULL: every walker) and
 *   site_map[s] != s; every other entry is exactly 0.0.  Closed walkers are skipped inside the contraction, a position at which the
 *   host's mirror of the MPO's states shows no open walker makes no trace launch; the right environment grows at every position.
 * The caches end as the per-call sequence leaves them: GetBTenLeftCol == N, GetBTenRightCol == 1.  Status PEPSGPU_EINVAL: NULL site_map
 * or out, a walker that is not UP; PEPSGPU_ERANGE: a map entry outside [0, phys_dim); PEPSGPU_ESTATE: no MPO set, an MPO given as
 * explicit tensors (it has no state to map), opp_level not in the DOWN stack, an active configuration override.  Every check runs before
 * a cache of the walker is released: a refused call leaves walker and context usable. */
int pepsgpu_walker_trace_slice(pepsgpu_ctx *ctx, int walker, int opp_level, const int32_t *site_map, const uint8_t *walker_mask,
                               double *out);
/* Completed pepsgpu_walker_trace_slice calls of this process (all contexts).  Needs no device. */
long pepsgpu_diag_walker_slice_calls(void);
/* The singlet-pair correlation <Delta^dag(ref bond) Delta(target bond)> of the t-J models (model_solvers/base/
 * singlet_pair_correlation_measurement_mixin.h:349-534; its MeasureSingletPairCorrelation :279-297 throws, the algorithm below it is
 * the one served here) on a FERMIONIC context: physical dimension 4 d, the walkers' configurations extended states e = s + d * variant
 * with the row-major variants 0 / 1 (the parity of the fermions up to and including the site).  The two sites of a horizontal bond are
 * adjacent in that order and a pair move keeps the parity of the pair, so only the variants of these two sites change and the rows
 * below need no change; the device derives them from occ [d] by the rule of pepsgpu_nn_pair_slice_fermion.
 *
 * The excited row of the reference bond (:376-401: the MPO of row y1 with the tensors of (x1, x1 + 1) replaced) without a host table:
 * the walker's MPO becomes row `num` under the walkers' current configurations with the pair (col, col + 1) replaced, per walker, by
 * candidate `slot` of pair_table ([d * d][2][2] over PHYSICAL states, the layout and the rules of pepsgpu_nn_pair_slice_fermion,
 * (-1, -1) for none); a walker without that candidate keeps its row.  A device-to-device copy of the configuration table plus ONE
 * two-site patch kernel, no upload, no synchronisation.  open_out [n] (may be NULL) = 1 where the walker has the candidate; sign_out [n]
 * (may be NULL) = Sigma(S') / Sigma(S) of the decoration, -1 where the fermion number changes by +-2, +1 where it is kept, 0 for none.
 * Afterwards the walker is exactly as after pepsgpu_walker_set_mpo(.., states, ..) with that row.  UP walkers only, d <= 8.
 * Status PEPSGPU_EINVAL: NULL occ or pair_table, a walker that is not UP, 4 * d != the physical dimension, an occ entry outside {0, 1},
 * slot outside {0, 1}, num outside the lattice or col + 1 outside the row, a table entry outside [-1, d), a candidate with only one -1
 * or one that changes the fermion parity of the pair; PEPSGPU_ESTATE: a state of the row with a column-major variant (2 / 3).  A refused
 * call leaves the walker and its MPO as they were. */
int pepsgpu_walker_set_mpo_excited_pair(pepsgpu_ctx *ctx, int walker, int num, int col, int d, const int32_t *occ, const int32_t *pair_table,
                                        int slot, uint8_t *open_out, int32_t *sign_out);
/* The target-row loop (:446-519 on bmps_walker.h:216-463) in one call with one read-back, for the walker's current MPO when that is a
 * row named by configuration or by states (N = cols >= 2):
 *   InitBTenLeft(opp, 0), InitBTenRight(opp, 1), then for x2 = 0 .. N - 2: TraceWithTwoSiteBTen at x2 with the states of (x2, x2 + 1)
 *   replaced by candidate k of pair_table, k = 0, 1, and ShiftBTenWindow(RIGHT) while x2 < N - 2.
 *   out [n][N - 1][2] (PEPSGPU_C128: interleaved (re, im)): entry (w, x2, k) = sign * trace * exp(log scales) as pair_out of
 *   pepsgpu_nn_pair_slice_fermion; exactly 0.0 for "no candidate" and where walker_mask[w] == 0 (NULL: every walker).
 * Every slot is traced with the launches of the per-call sequence in its order (two half steps and a dot, one candidate per walker), so
 * the numbers are the per-call path's; a slot for which the host's mirror of the MPO's states shows no open walker launches nothing,
 * closed walkers are skipped inside the chained float32 step and left zero by the store elsewhere; the window shifts at every position.
 * A table whose slot 0 maps (up, down) and (down, up) to themselves gives the unreplaced trace of those walkers (psi_original :460-476).
 * The caches end as the per-call sequence leaves them: GetBTenLeftCol == N - 2, GetBTenRightCol == N.
 * Status PEPSGPU_EINVAL: NULL occ, pair_table or out, a walker that is not UP, the table checks above; PEPSGPU_ESTATE: no MPO set, an
 * MPO given as explicit tensors, opp_level not in the DOWN stack, an active configuration override, a state of the row with a
 * column-major variant.  Every check runs before a cache of the walker is released: a refused call leaves walker and context usable. */
int pepsgpu_walker_pair_trace_slice(pepsgpu_ctx *ctx, int walker, int opp_level, int d, const int32_t *occ, const int32_t *pair_table,
                                    const uint8_t *walker_mask, double *out);
/* Completed pepsgpu_walker_pair_trace_slice calls of this process (all contexts).  Needs no device. */
long pepsgpu_diag_walker_pair_slice_calls(void);
/* The candidate kernel of pepsgpu_walker_pair_trace_slice and the patch kernel of pepsgpu_walker_set_mpo_excited_pair alone, on the
 * caller's extended rows ext [n][cols] (states in [0, 2 d)) for the pair (col, col + 1): cand_out [n][2][2] (slot, site) the extended
 * states under candidate k (the walker's own where it has none), skip_out [2][n] = 1 where the walker has no candidate k or
 * walker_mask[w] == 0 (NULL: none masked), sign_out [n][2] as above; patched_out [n][cols] the rows after the patch of `slot`.
 * Needs a device, no context. */
int pepsgpu_diag_walker_pair_cand(int cols, int d, const int32_t *occ, const int32_t *pair_table, int n, const int32_t *ext, int col,
                                  int slot, const uint8_t *walker_mask, int32_t *cand_out, int32_t *skip_out, int32_t *sign_out,
                                  int32_t *patched_out);
int pepsgpu_walker_evolve(pepsgpu_ctx *ctx, int walker);                                     /* Evolve(mpo)               :13-21  */
int pepsgpu_walker_evolve_step(pepsgpu_ctx *ctx, int walker);                                /* EvolveStep()              :23-49  */
int pepsgpu_walker_contract_row(pepsgpu_ctx *ctx, int walker, int opp_level, double *out);   /* ContractRow(mpo, opp)     :60-214 */
int pepsgpu_walker_init_bten(pepsgpu_ctx *ctx, int walker, int opp_level, int position, int target_col);   /* InitBTenLeft / Right :216-272 */
int pepsgpu_walker_grow_bten_step(pepsgpu_ctx *ctx, int walker, int opp_level, int position);   /* GrowBTenLeftStep / RightStep :274-324 */
int pepsgpu_walker_shift_bten_window(pepsgpu_ctx *ctx, int walker, int opp_level, int position);   /* ShiftBTenWindow       :326-350 */
/* TraceWithBTen(site, site_col, opp) :352-392 (two_site = 0) / TraceWithTwoSiteBTen(site_a, site_b, site_col, mpo, opp) :394-463
 * (two_site = 1).  The replacement site(s): site_states [n] ([n][2]) = SITPS component per walker, or site_tensors
 * [n_tensors] ([n_tensors][2]) [D^4] explicit (layout as above), or both NULL = the MPO's own tensors.  out [n]. */
int pepsgpu_walker_trace_with_bten(pepsgpu_ctx *ctx, int walker, int opp_level, int site_col, int two_site, const int32_t *site_states,
                                   const double *site_tensors, int n_tensors, double *out);
int pepsgpu_walker_clear_bten(pepsgpu_ctx *ctx, int walker);                                  /* ClearBTen()                       */
/* GetBMPS()[idx] of the walker (as pepsgpu_get_bmps_tensor) */
int pepsgpu_walker_get_bmps_tensor(pepsgpu_ctx *ctx, int walker, int idx, int *dims_out, double *data_out, double *logscale_out);
int pepsgpu_generate_bmps_approach(pepsgpu_ctx *ctx, int pos);  /* GenerateBMPSApproach      :11-17   */
int pepsgpu_bmps_stack_size(pepsgpu_ctx *ctx, int pos);         /* GetBMPS(pos).size(); <0 on error */
/* GetBMPS(pos)[level][idx]: dims_out[3]; data_out [n][d0*d1*d2] float64 (may be NULL);
 * logscale_out [n] (may be NULL): the BMPS represents tensors * exp(logscale). Gauge differs
 * from the reference (only gauge-invariant contractions are comparable). */
int pepsgpu_get_bmps_tensor(pepsgpu_ctx *ctx, int pos, int level, int idx, int *dims_out, double *data_out,
                            double *logscale_out);

/* BTen (rank-3 environments of one row/column) -- bmps_contractor_init.h:72-128, grow.h:243-373,:517-582 */
int pepsgpu_init_bten(pepsgpu_ctx *ctx, int pos, int slice);                               /* InitBTen      */
int pepsgpu_grow_full_bten(pepsgpu_ctx *ctx, int pos, int slice, int remain_sites, int init); /* GrowFullBTen */
int pepsgpu_grow_bten_step(pepsgpu_ctx *ctx, int pos);                                     /* GrowBTenStep  */
int pepsgpu_shift_bten_window(pepsgpu_ctx *ctx, int pos);                                  /* ShiftBTenWindow */
int pepsgpu_truncate_bten(pepsgpu_ctx *ctx, int pos, int length);                          /* TruncateBTen  */
int pepsgpu_bten_stack_size(pepsgpu_ctx *ctx, int pos);

/* Scalar contractions -- bmps_contractor_trace.h.  out_amp = [n] (or [n][n_cand]) float64. */
int pepsgpu_trace(pepsgpu_ctx *ctx, int row, int col, int bond_dir, double *out_amp);       /* Trace :11-28 */
/* ReplaceNNSiteTrace(tn, site_a, site_b, dir, T_a[cand[..][0]], T_b[cand[..][1]])  :90-205.
 * cand_states = [n][n_cand][2] physical states put on (site_a, site_b). */
int pepsgpu_replace_nn_trace(pepsgpu_ctx *ctx, int row, int col, int bond_dir, int n_cand,
                             const int32_t *cand_states, double *out_amp);
/* ReplaceOneSiteTrace(tn, site, T[cand], mps_orient)  :30-88.  cand_states = [n][n_cand]. */
int pepsgpu_replace_one_trace(pepsgpu_ctx *ctx, int row, int col, int mps_orient, int n_cand,
                              const int32_t *cand_states, double *out_amp);
/* BTen2 (rank-4 environments of two adjacent rows/columns, bten_set2_) -- bmps_contractor_init.h:130-186,
 * bmps_contractor_grow.h:375-527.  slice_num1 = the first of the two rows (LEFT/RIGHT) or columns (UP/DOWN). */
int pepsgpu_init_bten2(pepsgpu_ctx *ctx, int pos, int slice_num1);                              /* InitBTen2  init.h:130-186 */
int pepsgpu_grow_full_bten2(pepsgpu_ctx *ctx, int pos, int slice_num1, int remain_sites, int init); /* GrowFullBTen2 grow.h:375-470 */
int pepsgpu_grow_bten2_step(pepsgpu_ctx *ctx, int pos, int slice_num1);                         /* GrowBTen2Step grow.h:472-515 */
int pepsgpu_shift_bten2_window(pepsgpu_ctx *ctx, int pos, int slice_num1);                      /* ShiftBTen2Window grow.h:523-527 */
int pepsgpu_bten2_stack_size(pepsgpu_ctx *ctx, int pos);
/* Diagonal direction of a next-nearest / sqrt(5) link (basic.h:89-92 DIAGONAL_DIR). */
#define PEPSGPU_LEFTUP_TO_RIGHTDOWN 0
#define PEPSGPU_LEFTDOWN_TO_RIGHTUP 1
/* ReplaceNNNSiteTrace(tn, left_up_site, nnn_dir, mps_orient, ten_left, ten_right)  trace.h:207-324.
 * (row, col) = upper-left corner of the plaquette; cand_states = [n][n_cand][2] states put on the
 * (left, right) end of the diagonal.  n_cand = 0: no replacement (the plaquette trace), out = [n]. */
int pepsgpu_replace_nnn_trace(pepsgpu_ctx *ctx, int row, int col, int nnn_dir, int mps_orient, int n_cand,
                              const int32_t *cand_states, double *out_amp);
/* Environment-reusing diagonal (NNN) hop of a FERMIONIC state (square_spinless_fermion.h:161-213 through
 * square_nnn_energy_solver.h:203-265).  The reference's graded ReplaceNNNSiteTrace carries the fermionic signs in the tensor
 * algebra; in the sign-decorated form of this library a diagonal hop also changes the decoration (variant) of every site between
 * its two ends in the row-major mode order -- row r right of the plaquette, row r + 1 left of it -- so the hopped amplitude is a
 * local replacement against "twisted" two-row environments.  Three calls provide them:
 *   pepsgpu_bten2_select_set(ctx, set)        set = 0 / 1: the BTen2 set init / grow / shift / replace_* work on from now on
 *   pepsgpu_cfg_override_slice(ctx, orient, num, states)   states = [n][N] extended states the kernels read for row (HORIZONTAL) /
 *                                              column (VERTICAL) `num` instead of the walkers' own until cleared (states = NULL)
 *   pepsgpu_replace_plaquette_trace(ctx, row, col, n_cand, cand, left_set, right_set, out)   the plaquette with upper-left corner
 *                                              (row, col) closed with four replaced tensors, cand = [n][n_cand][4] states of
 *                                              (row, col), (row+1, col), (row+1, col+1), (row, col+1), between the LEFT BTen2 of
 *                                              `left_set` and the RIGHT BTen2 of `right_set`; n_cand = 0: the walkers' own states.
 * Any configuration update or set_configs drops the second set and the override. */
int pepsgpu_bten2_select_set(pepsgpu_ctx *ctx, int set);
int pepsgpu_cfg_override_slice(pepsgpu_ctx *ctx, int orient, int num, const int32_t *states);
int pepsgpu_replace_plaquette_trace(pepsgpu_ctx *ctx, int row, int col, int n_cand, const int32_t *cand_states, int left_set,
                                    int right_set, double *out_amp);
/* ReplaceTNNSiteTrace(tn, site0, mps_orient, T0, T1, T2)  trace.h:326-423.  (row, col) = first of
 * three consecutive sites along mps_orient; cand_states = [n][n_cand][3]. */
int pepsgpu_replace_tnn_trace(pepsgpu_ctx *ctx, int row, int col, int mps_orient, int n_cand,
                              const int32_t *cand_states, double *out_amp);
/* ReplaceSqrt5DistTwoSiteTrace(tn, left_up_site, sqrt5link_dir, mps_orient, ten_left, ten_right)
 * trace.h:425-536.  (row, col) = upper-left corner of the 2x3 (HORIZONTAL) or 3x2 (VERTICAL) block;
 * cand_states = [n][n_cand][2] states on the (left, right) end of the link. */
int pepsgpu_replace_sqrt5_trace(pepsgpu_ctx *ctx, int row, int col, int link_dir, int mps_orient, int n_cand,
                                const int32_t *cand_states, double *out_amp);
/* How pepsgpu_trace and the pepsgpu_replace_nn / one_trace calls scale their result on the way out.  A trace is kept as mantissa x exp(log-scale).
 * on_device == 0 (the default): the mantissas are read back and multiplied by std::exp(log-scale) on the host.  on_device != 0: they are
 * multiplied by exp(log-scale) in a kernel, the expression the device-side slices use, so that a per-bond hook path returns the bits of
 * the slice that replaces it (the two exponentials may differ in the last bit; SquareHubbardModel::EvaluateBondEnergy and the hook of
 * MCUpdateSquareNNHubbardU1U1OBC switch it on around their calls).  The other trace calls keep the host form. */
int pepsgpu_trace_scaling(pepsgpu_ctx *ctx, int on_device);
/* PunchHole(tn, site, mps_orient)  grow.h:150-183.  out = [n][D][D][D][D] float64 (legs L,D,R,U, zero padded). */
int pepsgpu_punch_hole(pepsgpu_ctx *ctx, int row, int col, int mps_orient, double *out);
/* out == NULL: the hole of every walker stays on the device (resident hole store) for
 * pepsgpu_grad_accumulate.  The three calls below replace the per-sample accumulation loop
 * Ostar_sum += O*, ELocConj_Ostar_sum += E_loc^* O* (mc_energy_grad_evaluator.h:257-278; exact
 * summation: exact_summation_energy_evaluator.h:218-239) without moving the holes over PCIe:
 *   O*(site)[config_w(site)] = hole_w(site) / psi_w            (exact_sum = 0, weight 1)
 *   |psi|^2 O*               = psi_w * hole_w(site)            (exact_sum = 1)
 * psi, eloc = [n] host arrays (the solver's scalars).  pepsgpu_grad_read returns S_O and S_EO in the
 * state layout [row][col][s][L][D][R][U]; the cross-rank mean is one all-reduce of those buffers
 * (replaces MPIMeanTensor, statistics_tensor.h:37-79). */
int pepsgpu_grad_reset(pepsgpu_ctx *ctx);
int pepsgpu_grad_accumulate(pepsgpu_ctx *ctx, const double *psi, const double *eloc, int exact_sum);
/* The same with the component every hole belongs to named by the caller: states = [n][rows][cols], 0 <= state < d of
 * the context (NULL: the walkers' current configuration, as above).  Fermionic states (sign-decorated components,
 * INTEGRATION.md): the holes are those of the row-major decoration, states = the extended states of that decoration and
 * psi = the plain contraction value, whatever mode order the walkers have been moved to since the holes were punched
 * (replaces the same loop, mc_energy_grad_evaluator.h:257-278, for fermionic tensors). */
int pepsgpu_grad_accumulate_states(pepsgpu_ctx *ctx, const double *psi, const double *eloc, int exact_sum,
                                   const int32_t *states);
int pepsgpu_grad_read(pepsgpu_ctx *ctx, double *s_o_out, double *s_eo_out);

/* Stochastic reconfiguration: the O* samples stay in HBM and the S-matrix product of
 * SRSMatrix::operator* (optimizer/stochastic_reconfiguration_smatrix.h:37-99) is two sweeps over them.
 *   pepsgpu_sr_begin(max_samples)   allocate the store [sample][site][D^4]
 *   pepsgpu_sr_append(psi)          append O*_w = hole_w / psi_w of the current walkers (resident hole store of
 *                                   pepsgpu_punch_hole(.., NULL); replaces Ostar_samples.push_back, mc_energy_grad_evaluator.h:270)
 *   pepsgpu_sr_sum(out)             sum_i O*_i in the state layout (the caller divides by the total sample count -> Ostar_mean)
 *   pepsgpu_sr_matvec(v, mean_dot_v, scale, out)   out = scale * sum_i (O*_i . v - mean_dot_v) O*_i  (state layout, float64);
 *                                   the caller all-reduces over ranks and adds diag_shift * v. */
int pepsgpu_sr_begin(pepsgpu_ctx *ctx, int max_samples);
int pepsgpu_sr_append(pepsgpu_ctx *ctx, const double *psi);
int pepsgpu_sr_count(pepsgpu_ctx *ctx);
int pepsgpu_sr_sum(pepsgpu_ctx *ctx, double *sum_out);
int pepsgpu_sr_matvec(pepsgpu_ctx *ctx, const double *v, double mean_dot_v, double scale, double *out);
/* PEPSGPU_C128 contexts (SRSMatrix<QLTEN_Complex, QNT>): the sample store (begin / append / sum) takes psi and returns sums as
 * interleaved pairs; O*_i = conj(1 / psi_i) Dag(hole_i) (mc_energy_grad_evaluator.h:245-270); the product uses the positive-definite
 * pairing of SplitIndexTPS::operator* (split_index_tps.h:370-377):  out = scale * sum_i (<O*_i, v> - mean_dot_v) O*_i,
 * <a, b> = sum conj(a) b; v, out = state layout, interleaved pairs.  pepsgpu_sr_cg_solve works on PEPSGPU_C128 contexts too (b, x0, x_out
 * interleaved pairs; pap valid when Re > 0 and |Im| < 1e-10 as detail::pap_is_valid), and so do the MinSR blocks: pepsgpu_sr_gram returns
 * ip_ij = O*_i * O*_j = sum conj(O*_i) O*_j as interleaved pairs, pepsgpu_sr_weighted_sum takes complex weights (interleaved). */
int pepsgpu_sr_matvec_c128(pepsgpu_ctx *ctx, const double *v, double mean_dot_v_re, double mean_dot_v_im, double scale, double *out);
/* ConjugateGradientSolver (utility/conjugate_gradient_solver.h:181-276) on (S + diag_shift) x = b over the samples of THIS
 * context, every vector resident in HBM; parameters = ConjugateGradientParams (optimizer/optimizer_params.h:50-57).
 * b, x0 (NULL = 0) and x_out are host buffers in the state layout.  reason = CGTerminationReason:
 * 0 converged, 1 max iterations, 2 indefinite matrix, 3 numerical breakdown, 4 stagnated; on 1..4 x_out is the best iterate.
 * Multi-rank solves go through pepsgpu_sr_matvec + an all-reduce per product (peps_amd/sr.py). */
int pepsgpu_sr_cg_solve(pepsgpu_ctx *ctx, const double *b, const double *x0, double diag_shift, int max_iter,
                        double relative_tolerance, double absolute_tolerance, int residual_recompute_interval,
                        double orthogonality_threshold, double *x_out, double *residual_norm, int *iterations, int *reason);
/* MinSR building blocks (optimizer/minsr_tmatrix.h:53-147, optimizer_impl.h:1126-1215):
 *   pepsgpu_sr_gram          out[i][j] = <O*_i, O*_j'>, i over the local samples, j over a batch of n_remote samples given by
 *                            DEVICE pointers (layout of the local store: [sample][site][D^4] of the context's dtype and
 *                            int32 [sample][site]); remote == NULL: the local batch against itself.  One MFMA GEMM, f64 sums.
 *   pepsgpu_sr_weighted_sum  out = sum_i y[i] O*_i over the local samples (state layout) -- the back-substitution
 *   pepsgpu_sr_copy_samples  device-to-device copy of the local store into caller-owned device buffers (what the ring
 *                            exchange of MinSRTMatrix::Construct sends to the next rank) */
int pepsgpu_sr_gram(pepsgpu_ctx *ctx, const void *remote_samples_dev, const int32_t *remote_configs_dev, int n_remote, double *out);
int pepsgpu_sr_weighted_sum(pepsgpu_ctx *ctx, const double *y, double *out);
int pepsgpu_sr_copy_samples(pepsgpu_ctx *ctx, void *dst_samples_dev, int32_t *dst_configs_dev);

/* Device-resident optimisation step: the first-order update rules of optimizer/optimizer_impl.h and the one-rank SR step on
 * buffers that stay in HBM.  Master parameters theta, the gradient / direction g and the rule state (velocity, m1, m2, acc, the
 * Adam timestep) are float64 -- interleaved complex float64 on a PEPSGPU_C128 context; m2 and acc are real there too -- in the
 * layout of S_O / S_EO, and are freed with the context.  Host buffers of these calls use the padded layout of
 * pepsgpu_state_upload ([row][col][s][L][D][R][U], float64 / interleaved pairs).  Every call that rewrites the device state
 * (opt_step, opt_scale_state) leaves the walkers' environments stale exactly as pepsgpu_state_upload does: re-initialise with
 * pepsgpu_walkers_set_configs.  Status: PEPSGPU_ESTATE before pepsgpu_opt_begin (and for opt_begin without a state, opt_natural_gradient
 * with an empty sample store, opt_gradient_from_accumulators with nothing accumulated); PEPSGPU_EINVAL for a non-finite or negative
 * lr, an unknown rule, a wrong n_params, a non-finite or negative rule parameter, an Adam beta outside [0, 1), weight_sum <= 0, a
 * NULL buffer.  A refused call leaves theta, the rule state and the device state untouched.
 *   pepsgpu_opt_begin      theta <- double(device state), device to device; clears the rule state.  Call again after a
 *                          pepsgpu_state_upload to adopt the uploaded state.
 *   pepsgpu_opt_end        frees the optimizer buffers.
 *   pepsgpu_opt_gradient_from_accumulators
 *                          g <- (S_EO - conj(E) S_O) / W with E = e_loc_sum / weight_sum (e_loc_sum: 1 double, 2 on a complex context)
 *                          from the resident accumulators: GradAccumulatorT::Finish / exact_summation_energy_evaluator.h:286-295 without
 *                          pepsgpu_grad_read.  energy_out (1 or 2 doubles) and grad_norm_out = sqrt(sum |g|^2) may be NULL.  The norm is a
 *                          two-stage sum in a fixed order: equal accumulators give bit-identical norms.
 *   pepsgpu_opt_set_gradient / pepsgpu_opt_get_gradient
 *                          g from / to the host (what a caller with its own gradient, or a test, needs).
 *   pepsgpu_opt_clip       optimizer_impl.h:311-316: first the element-wise clip (clip_value > 0: real sign(x) min(|x|, c), complex
 *                          x min(1, c / |x|)), then ClipByGlobalNorm (split_index_tps_impl.h:573-580; clip_norm > 0: g *= clip_norm / r
 *                          only if r > clip_norm, r taken after the element-wise clip).  norm_before_out (nullable) = sqrt(sum |g|^2) on entry.
 *   pepsgpu_opt_natural_gradient
 *                          StochasticReconfigurationUpdate's solve on one rank (optimizer_impl.h, SR branch): the loop of
 *                          pepsgpu_sr_cg_solve with b = g, x0 = 0 read and the solution written in HBM, g <- x.
 *                          direction_norm_out (nullable) = sqrt(sum |x|^2).  Multi-rank: peps_amd/sr.py.
 *   pepsgpu_opt_step       one fused pass: theta, rule state and device state = T(theta).  rule 0 SGD (optimizer_impl.h:949-990), params
 *                          (momentum, nesterov != 0, weight_decay); 1 AdaGrad (:1252-1307), params (epsilon, initial_accumulator_value:
 *                          taken at the first AdaGrad step after opt_begin); 2 Adam (:1327-1396), params (beta1, beta2, epsilon,
 *                          weight_decay).  ElementWiseInv(eps) = 1 / (x + eps) in both.
 *   pepsgpu_opt_scale_state theta *= factor, device state = T(theta): the `*= scale_factor_on_site` of NormalizeStateOrder1
 *                          (monte_carlo_engine.h:206-240).
 *   pepsgpu_opt_read_state theta to the host.
 *
 * Fermionic states.  A fermionic state lives on the device as 4 d decorated components per site, T''[s + d var] = sigma_var * T[s]
 * =: E T (peps_amd/fermion.py; sigma_0 = 1, sigma_1 = (-1)^u, sigma_2 = (-1)^base, sigma_3 = (-1)^(base + l), base = u n_s + u + dn r +
 * l + l u over the bond parities l, dn, r, u of the element and the parity n_s of the stored state; an element is a parameter iff
 * l + dn + r + u + n_s is even).  pepsgpu_fermion_decoration_set tells the context so: d stored states with parities nf[d] and the
 * bond parities bond_parity [rows][cols][4][D] (legs L, D, R, U; entries past a leg's true dimension are ignored).  d = 0 clears the
 * decoration.  PEPSGPU_EINVAL: phys_dim != 4 d, a parity outside {0, 1}, or optimizer buffers exist (pepsgpu_opt_end first).
 * With a decoration set every optimizer vector stays in the extended layout and in the range of E, and the calls above become
 *   opt_begin               additionally checks theta == Pi(theta) / 4 element by element (Pi = E mask E^T), exact for a decorated
 *                           state; otherwise PEPSGPU_EINVAL names the first offending site and no buffer is kept.
 *   opt_gradient_from_accumulators   g <- Pi (S_EO - conj(E) S_O) / W, i.e. E of the folded gradient (fermion.fold_gradient); grad_norm_out
 *                           is the norm over the STORED parameters, 1/2 of the extended one.
 *   opt_set_gradient        takes the derivative with respect to the extended components (padded extended layout) and applies Pi;
 *   opt_get_gradient / opt_read_state return E g / E theta in the same layout: components 0 .. d - 1 (variant 0) are the stored arrays.
 *   opt_clip                compares and reports the stored norm; the element-wise clip and the scale factor are unchanged.
 *   opt_natural_gradient    solves (E^T S_ext E + diag_shift) x = g in the stored parameters: Pi is applied to every S v and the dot
 *                           products are scaled to the stored ones; residual_norm and direction_norm_out are stored norms.
 *   opt_step / opt_scale_state   unchanged: element-wise, so a step on (E theta, Pi g) is bit for bit E of the step on (theta, E^T g).
 * pepsgpu_sr_cg_solve (host vectors) ignores the decoration. */
int pepsgpu_opt_begin(pepsgpu_ctx *ctx);
int pepsgpu_opt_end(pepsgpu_ctx *ctx);
int pepsgpu_opt_gradient_from_accumulators(pepsgpu_ctx *ctx, const double *e_loc_sum, double weight_sum, double *energy_out,
                                           double *grad_norm_out);
int pepsgpu_opt_set_gradient(pepsgpu_ctx *ctx, const double *host);
int pepsgpu_opt_get_gradient(pepsgpu_ctx *ctx, double *host);
int pepsgpu_opt_clip(pepsgpu_ctx *ctx, double clip_value, double clip_norm, double *norm_before_out);
int pepsgpu_opt_natural_gradient(pepsgpu_ctx *ctx, double diag_shift, int max_iter, double relative_tolerance, double absolute_tolerance,
                                 int residual_recompute_interval, double orthogonality_threshold, double *residual_norm, int *iterations,
                                 int *reason, double *direction_norm_out);
int pepsgpu_opt_step(pepsgpu_ctx *ctx, int rule, double lr, const double *params, int n_params);
int pepsgpu_opt_scale_state(pepsgpu_ctx *ctx, double factor);
int pepsgpu_opt_read_state(pepsgpu_ctx *ctx, double *host);
int pepsgpu_fermion_decoration_set(pepsgpu_ctx *ctx, int d, const int32_t *nf, const uint8_t *bond_parity);

/* The lowest-energy parameters of a VMC run, kept in HBM: VMCPEPSOptimizer's tps_lowest_ (vmc_peps_optimizer_impl.h:118-121), which
 * the reference copies on the host whenever an iteration's energy is below the minimum so far.
 *   pepsgpu_vmc_snapshot_save   device-to-device copy of theta (the master parameters of pepsgpu_opt_begin) into a buffer of its own,
 *                               allocated on first use; a later save overwrites it.  The buffer is freed by pepsgpu_opt_end, by a new
 *                               pepsgpu_opt_begin and with the context.  Neither theta, the rule state nor the device state is touched.
 *   pepsgpu_vmc_snapshot_read   the snapshot to the host in the layout of pepsgpu_opt_read_state (padded [row][col][s][L][D][R][U],
 *                               float64 / interleaved pairs); under a fermionic decoration it is E theta as saved, components 0 .. d - 1
 *                               (variant 0) are the stored arrays, exactly as pepsgpu_opt_read_state returns theta.
 *   pepsgpu_vmc_snapshot_clear  frees the buffer (no snapshot afterwards; clearing twice is fine).
 * Status: PEPSGPU_ESTATE before pepsgpu_opt_begin (all three) and for a read without a snapshot; PEPSGPU_EINVAL for a NULL buffer.  A
 * refused call leaves the context usable and a held snapshot untouched.
 * The prefix is not pepsgpu_opt_: the set of pepsgpu_opt_* entries is closed. */
int pepsgpu_vmc_snapshot_save(pepsgpu_ctx *ctx);
int pepsgpu_vmc_snapshot_read(pepsgpu_ctx *ctx, double *host);
int pepsgpu_vmc_snapshot_clear(pepsgpu_ctx *ctx);

/* The base of a step, kept in HBM: what the spike rollback and the step selectors of the reference's Optimizer do with host copies
 * of the SplitIndexTPS.  One more vector with the extents of theta; no tensor crosses PCIe.
 *   pepsgpu_guard_base_save     `prev_accepted_state_ = current_state` (optimizer_impl.h:838-841) and the base of the selector trials
 *                               (:320-542): device-to-device copy of theta into a buffer of its own, allocated on first use; a later
 *                               save overwrites it.  Freed by pepsgpu_opt_end, by a new pepsgpu_opt_begin and with the context.
 *   pepsgpu_guard_base_restore  `current_state = prev_accepted_state_` (the rollback, :1868-1973) and the end of a selector trial:
 *                               theta <- base, device state = T(base) in one pass.  The gradient buffer is not an operand: after a
 *                               spike it may hold Inf / NaN.  theta is bit for bit the saved one and the device state is what
 *                               pepsgpu_opt_begin or a step would have written for it.  The rule state is not touched.
 *   pepsgpu_guard_base_clear    `has_prev_state_ = false`: no base afterwards; the buffer stays.
 *   pepsgpu_guard_preview       SGDPreviewUpdate_ (:1001): theta <- the SGD rule of pepsgpu_opt_step applied to the *base* with the
 *                               current g, device state = T(theta).  The velocity is read and not written.  rule must be 0; params
 *                               (momentum, nesterov != 0, weight_decay) as for pepsgpu_opt_step.  With (0, 0, 0) it is
 *                               base - lr g: the trial along the SR / MinSR direction that pepsgpu_opt_natural_gradient /
 *                               pepsgpu_minsr_direction left in g.  On the same base it leaves theta and the device state bit for
 *                               bit as pepsgpu_opt_step(0, lr, params) leaves them (one device function holds the arithmetic).
 * Status: PEPSGPU_ESTATE before pepsgpu_opt_begin (all four) and for a restore / preview without a saved base; PEPSGPU_EINVAL for a
 * rule other than 0 and for the parameter errors of pepsgpu_opt_step.  A refused call leaves the context and a saved base untouched.
 * Under a fermionic decoration the base is E theta as saved and both passes run unchanged.
 * The prefix is not pepsgpu_opt_: the set of pepsgpu_opt_* entries is closed. */
int pepsgpu_guard_base_save(pepsgpu_ctx *ctx);
int pepsgpu_guard_base_restore(pepsgpu_ctx *ctx);
int pepsgpu_guard_base_clear(pepsgpu_ctx *ctx);
int pepsgpu_guard_preview(pepsgpu_ctx *ctx, int rule, double lr, const double *params, int n_params);

/* MinSR inside the device-resident optimizer: Optimizer::CalculateMinSRDirection_ on one rank (optimizer/optimizer_impl.h:1126-1215,
 * minsr_tmatrix.h:53-147, minsr_eigensolve.h:44-155; parameters = MinSRParams, optimizer_params.h:220-232).  With Ns = pepsgpu_sr_count
 * samples in the store, everything that scales with Ns^2 or with the parameter count stays in HBM:
 *   1  raw Gram of the resident O* store (the GEMM of pepsgpu_sr_gram, f64 sums, summed and mirrored on the device);
 *   2  T_ij = (G_ij - m_i - conj(m_j) + c) / Ns, m_i = sum_j G_ij / Ns, c = sum_i m_i / Ns (minsr_tmatrix.h:141-147);
 *   3  T = Z diag(w) Z^H by a two-sided parallel Jacobi method in HBM (csrc/eigh_jacobi.h; float64 or complex whatever the context);
 *   4  ApplyPseudoInverseCutoff (minsr_eigensolve.h:44-78): cutoff = r_pinv max|w| + a_pinv; soft_cutoff != 0: f = w^5 / (w^6 + cutoff^6),
 *      0 where the denominator is 0; else f = 1 / w where |w| > cutoff, 0 elsewhere;
 *   5  y = Z f(w) Z^H eps_bar, eps_bar_i = conj(E_i - E) / Ns (optimizer_impl.h:1139-1146);
 *   6  g <- sum_i y_i O*_i - (sum_i y_i) (sum_i O*_i) / Ns into the optimizer's direction buffer (the kernels of
 *      pepsgpu_sr_weighted_sum / pepsgpu_sr_sum, device to device);
 *   7  direction_norm_out (nullable) = sqrt(sum |g|^2), the two-stage fixed-order sum of the optimizer.
 * eloc = the Ns local energies in the order the samples were appended (Ns doubles, 2 Ns interleaved on a PEPSGPU_C128 context), energy
 * = their mean (1 or 2 doubles).  info_out (nullable, 4 doubles) = [max|w|, cutoff, number of eigenvalues with |w| > cutoff, Jacobi
 * sweeps].  pepsgpu_opt_step(ctx, 0, lr, {0, 0, 0}, 3) then applies theta -= lr g, as for the SR step.  Works on PEPSGPU_F32, F64 and C128
 * contexts (the store has the context's dtype).  The scratch (T and Z: 2 Ns^2 doubles, twice that on a complex context) is allocated on
 * first use and freed by pepsgpu_opt_end or with the context.
 * Status: PEPSGPU_ESTATE before pepsgpu_opt_begin or with an empty sample store; PEPSGPU_EINVAL for a NULL eloc / energy, a non-finite
 * or negative r_pinv / a_pinv, a non-finite energy or local energy, or when a fermionic decoration is set (T in the stored parameters
 * under the decoration is a follow-up, as is the multi-rank T matrix: peps_amd/sr.py stays the multi-rank path); PEPSGPU_ENOCONV when the
 * eigensolver reaches its cap of 30 sweeps.  A refused call leaves g, theta and the device state untouched.
 * The prefix is not pepsgpu_opt_: the set of pepsgpu_opt_* entries is closed.
 *
 * pepsgpu_diag_eigh runs the eigensolver alone on the context's device: a = n x n row-major host matrix, real symmetric or (is_complex
 * != 0, interleaved pairs) complex Hermitian; w_out[n] ascending, z_out = n x n row-major with the eigenvector of w[k] in column k,
 * sweeps_out (nullable) = sweeps run, the closing one that rotated nothing included.  PEPSGPU_EINVAL: n < 1, a NULL buffer, a
 * non-finite entry; PEPSGPU_ENOCONV at the sweep cap (the outputs then hold the state reached). */
int pepsgpu_minsr_direction(pepsgpu_ctx *ctx, const double *eloc, const double *energy, double r_pinv, double a_pinv, int soft_cutoff,
                            double *direction_norm_out, double *info_out);
int pepsgpu_diag_eigh(pepsgpu_ctx *ctx, int n, int is_complex, const double *a, double *w_out, double *z_out, int *sweeps_out);

/* L-BFGS inside the device-resident optimizer (optimizer/optimizer_impl.h; parameters = LBFGSParams, optimizer_params.h:119-152).  The
 * history ring of (s_i, y_i), the anchor (theta_a, g_a), the search direction d and the base (theta_b, g_b) of the current line search
 * live in HBM in the layout of theta; a trial point of a line search costs one element-wise pass and one dot product, the evaluator then
 * runs on the resident state.  Inner products are RealInnerProduct_ (:1398-1401): the plain dot over the doubles, interleaved pairs on
 * a PEPSGPU_C128 context; under a fermionic decoration they are those of the stored parameters.  Reductions have a fixed order: the same
 * call on the same buffers returns the same bytes.
 *   pepsgpu_lbfgs_begin    allocates and zeroes the buffers for history_size pairs, 1 <= history_size <= 32 (ResetLBFGSState_,
 *                          :1404-1413; the reference refuses 0).  pepsgpu_lbfgs_end frees them; so do pepsgpu_opt_end and a new pepsgpu_opt_begin.
 *   pepsgpu_lbfgs_reset    drops history, anchor and pending direction and zeroes the counters; the buffers stay.
 *   pepsgpu_lbfgs_update   UpdateLBFGSHistoryFromAnchor_ (:1443-1486) from theta and the gradient buffer.  Without an anchor: nothing
 *                          (*outcome = 0).  Else s = theta - theta_a, y = g - g_a, curvature = <s,y>; curvature <= min_curvature with
 *                          use_damping and <y,y> > DBL_EPSILON: y += (delta / <y,y>) s, delta = min_curvature - curvature + 1e-15, and the
 *                          curvature is taken again.  curvature <= min_curvature still: skipped (*outcome = 3), else pushed, evicting
 *                          the oldest pair beyond history_size (*outcome = 1, 2 after damping).  *curvature = the last value.
 *   pepsgpu_lbfgs_direction  ComputeLBFGSSearchDirection_ (:1488-1532): two-loop recursion with gamma = <s,y> / <y,y> of the newest pair
 *                          (1 unless <y,y> > DBL_EPSILON and <s,y> > min_curvature), evaluated in the coefficients of [s_i, y_i, g] on
 *                          the host in double from the inner products; the norm cap (max_direction_norm > 0: d *= max / |d| beyond
 *                          it); the descent guard (:620-641): <g,d> >= 0 drops history and anchor and takes d = -g (*was_reset = 1).
 *                          *dphi0 = <g,d>, *norm = |d|.  Records the base of the search: theta_b <- theta, g_b <- g.
 *   pepsgpu_lbfgs_trial    theta = theta_b + alpha d and device state = T(theta) in one pass (:1581-1585, ApplyFixedLBFGSStep_
 *                          :1534-1545); alpha = 0 restores theta_b bit for bit.
 *   pepsgpu_lbfgs_slope    *dphi = <g, d> of the current gradient buffer (:1590).
 *   pepsgpu_lbfgs_commit   the anchor becomes (theta_b, g_b) (:847-850; pointer exchange); the direction is consumed.
 *   pepsgpu_lbfgs_get_direction / pepsgpu_lbfgs_get_pair   d / pair `index` of the history (0 = oldest; either output nullable) to the
 *                          host in the upload layout, as pepsgpu_opt_get_gradient.
 *   pepsgpu_lbfgs_counters out4 = [skipped pairs, damped pairs, descent resets, pairs in the history].  The descent-reset counter
 *                          survives the reset it counts (the reference's own reset zeroes it).
 * Status: PEPSGPU_ESTATE before pepsgpu_opt_begin (lbfgs_begin) / before pepsgpu_lbfgs_begin (all others), and for trial / slope /
 * commit without a direction; PEPSGPU_EINVAL for a history_size outside [1, 32], a NaN parameter, a negative or non-finite alpha;
 * PEPSGPU_ERANGE for an index outside the history.  A refused call leaves theta, g and the history untouched.
 * The prefix is not pepsgpu_opt_, and L-BFGS is not a rule id of pepsgpu_opt_step: both sets are closed. */
int pepsgpu_lbfgs_begin(pepsgpu_ctx *ctx, int history_size);
int pepsgpu_lbfgs_end(pepsgpu_ctx *ctx);
int pepsgpu_lbfgs_reset(pepsgpu_ctx *ctx);
int pepsgpu_lbfgs_update(pepsgpu_ctx *ctx, double min_curvature, int use_damping, int *outcome, double *curvature);
int pepsgpu_lbfgs_direction(pepsgpu_ctx *ctx, double min_curvature, double max_direction_norm, double *dphi0, double *norm,
                            int *was_reset);
int pepsgpu_lbfgs_trial(pepsgpu_ctx *ctx, double alpha);
int pepsgpu_lbfgs_slope(pepsgpu_ctx *ctx, double *dphi);
int pepsgpu_lbfgs_commit(pepsgpu_ctx *ctx);
int pepsgpu_lbfgs_get_direction(pepsgpu_ctx *ctx, double *out);
int pepsgpu_lbfgs_get_pair(pepsgpu_ctx *ctx, int index, double *s_out, double *y_out);
int pepsgpu_lbfgs_counters(pepsgpu_ctx *ctx, long *out4);

/* TPSWaveFunctionComponent::UpdateLocal (wave_function_component.h:345-378) for the walkers with
 * accept_mask[w] != 0 (NULL = all): config(site_k) = new_states[w][k], tn.UpdateSiteTensor,
 * contractor.EraseEnvsAfterUpdate(site_k) (trace.h:538-589).  sites = [n_sites][2] (row, col). */
int pepsgpu_update_local(pepsgpu_ctx *ctx, int n_sites, const int32_t *sites, const int32_t *new_states,
                         const uint8_t *accept_mask);
int pepsgpu_erase_envs_after_update(pepsgpu_ctx *ctx, int row, int col);                   /* trace.h:538-589 */

/* TPSWaveFunctionComponent::EvaluateAmplitude (wave_function_component.h:187-212):
 * GrowBMPSForRow(0); GrowFullBTen(RIGHT,0,2,true); InitBTen(LEFT,0); Trace({0,0},HORIZONTAL). */
int pepsgpu_evaluate_amplitude(pepsgpu_ctx *ctx, double *out_amp);

/* walker_flags[w] != 0: a boundary tensor of walker w vanished (reference throws, bmps_impl.h:839-843). */
int pepsgpu_walker_flags(pepsgpu_ctx *ctx, int32_t *flags_out);
int pepsgpu_sync(pepsgpu_ctx *ctx);
/* stats_out: [0] row absorptions, [1] Jacobi launches, [2] Jacobi sweeps (sum of per-launch maxima), [3] device bytes held,
 * [4] largest sweep count; with PEPSGPU_DEBUG_SWEEPS=1 at context creation also [5] sum of live carry rows, [6] sum of
 * carry sizes, [7] largest live carry of any walker (> 32: the dense Gram / Cholesky / full Jacobi route ran); [8] absorptions
 * done twice (a bond sized from the previous row's live count was filled, or a kernel size class skipped on the previous row's
 * carry rank was needed after all: performance hints only, results never depend on them) */
int pepsgpu_stats(pepsgpu_ctx *ctx, double *stats_out, int n);
/* Per-kernel timing with HIP events recorded on the launch stream (bench.py roofline leg).
 * out = [11][5]: {ms, launches, algorithmic flops, executed flops, operand + result bytes of the live extents} per category
 * 0 contraction GEMMs, 1 f64 Gram, 2 Cholesky, 3 Jacobi, 4 select, 5 normalise, 6 BTen/trace GEMMs, 7 Jacobi of edge blocks,
 * 8 Gram + Cholesky of the preconditioned truncation (mid-rank route), 9 its back-multiplication, 10 the chained contraction
 * kernel alone (tgemm_chain_kernel: one bracket per launch of that kernel; NOT included in category 0).
 * "algorithmic" = flops of the reference op the launch replaces (SURVEY.md 8d formulas). */
int pepsgpu_profile_enable(pepsgpu_ctx *ctx, int on);
int pepsgpu_profile_read(pepsgpu_ctx *ctx, double *out);

/* ---- the one exchange step of the path: sum over ranks of the energy / gradient accumulators ----
 * Replaces MPIMeanTensor per (site, component) (monte_carlo_tools/statistics_tensor.h:37-79), the
 * MPI_Send/Recv + reduce of S_O, S_EO (exact_summation_energy_evaluator.h:252-280, mc_energy_grad_evaluator.h:292-310),
 * the energy Gather (statistics.h:185-207) and the MPI_Allreduce(MAX) of acceptance rates
 * (mc_energy_grad_evaluator.h:405-410) by RCCL all-reduces over xGMI, one rank (= one context) per GPU.
 * The reference host owns the rendezvous (it has MPI): rank 0 calls pepsgpu_comm_unique_id and broadcasts the 128
 * bytes (MPI_Bcast; torch.distributed.broadcast_object_list in the Python host), every rank calls pepsgpu_comm_init.
 * A context without a communicator is a single rank: every reduction is the identity (as MPI with one rank). */
int pepsgpu_comm_unique_id(void *id128_out);                                     /* ncclGetUniqueId: 128 bytes */
int pepsgpu_comm_init(pepsgpu_ctx *ctx, int nranks, int rank, const void *id128); /* collective over the ranks */
int pepsgpu_comm_size(pepsgpu_ctx *ctx);
int pepsgpu_comm_rank(pepsgpu_ctx *ctx);
int pepsgpu_comm_destroy(pepsgpu_ctx *ctx);
/* in-place all-reduce of n elements on the context's stream, complete on return.  dtype: 0 f32, 1 f64, 2 int32;
 * op: 0 sum, 1 max; on_device != 0: buf is an HBM pointer of this context's GPU (no host hop), else a host buffer
 * staged through HBM. */
int pepsgpu_allreduce(pepsgpu_ctx *ctx, void *buf, long n, int dtype, int op, int on_device);
/* S_O and S_EO of pepsgpu_grad_accumulate summed over the ranks where they live (HBM), before pepsgpu_grad_read. */
int pepsgpu_grad_allreduce(pepsgpu_ctx *ctx);
/* Broadcast of the parameter buffer after an optimizer update: the flat SITPS of rank `root` (pepsgpu_state_upload there)
 * goes to the HBM state buffer of every rank of the context's communicator with one ncclBroadcast over xGMI -- no host upload
 * on the other ranks.  Replaces the per-tensor MPI_Bcast of SplitIndexTPS (two_dim_tn/tps/split_index_tps_impl.h:778-880,
 * called at algorithm/vmc_update/mc_energy_grad_evaluator.h:161).  Collective over the ranks; one rank: marks the state valid. */
int pepsgpu_bcast_state(pepsgpu_ctx *ctx, int root);
/* device pointers of the two float64 accumulators ([row][col][s][D^4 slot], n_elems each) for hosts that run their own
 * collective on them (torch.distributed backend "nccl" = RCCL: peps_amd/dist.py wraps them without a copy). */
int pepsgpu_grad_device_ptr(pepsgpu_ctx *ctx, void **so_dev, void **seo_dev, long *n_elems);

/* ---- diagnostics (unit tests of the kernels; not part of the reference surface) ---- */
int pepsgpu_diag_tgemm(int dtype_in, int dtype_out, const int *desc_ints, int n_ints, const void *A, size_t a_elems,
                       const void *B, size_t b_elems, void *C, size_t c_elems, int nbatch, long wA, long wB, long wC);
/* the whole tensor-GEMM descriptor (tgemm.h TGemmDesc) through tgemm_launch, for the kernel tests.
 * types: (A, B, C, accumulation) = 0 f32/f32/f32/f32, 1 f32/f32/f32/f64, 2 f32/f32/f64/f64, 3 f64 x 4, 4 c128 x 4.
 * desc_ints[89]: 0..26 I, J, K, sAi, sAk, sBk, sBj, sCi, sCj (3 each); then for dI[0..2], dJ[0..2], dK[0..2] (9 each):
 * 27 pool offset of p (-1 = none), 36 mul, 45 mask, 54 div; 63 dynI, 64 dynK (pool offsets), 65 dynI_mul, 66 dynK_mul,
 * 67 selA, 68 selB (pool offsets), 69 selA_inc, 70 selB_inc, 71 bdivA, 72 bdivB, 73 bdivC, 74 seldivA, 75 seldivB, 76 nbatch,
 * 77 accumulate, 78 upper_only, 79 conjA, 80 conjB, 81 batch_flag (pool offset), 82 prefer_tiled, 83 acc64, 84 scale_out on,
 * 85 norm_log on, 86 norm_flag on, 87 scale_in on, 88 reserved (0).  desc_longs[5] = wA, wB, wC, selA_mul, selB_mul;
 * desc_dbls[1] = alpha.  pool = the per-batch int arrays the offsets point into; scale_in / scale_out / norm_log / norm_flag:
 * nbatch each (the last three in/out).  The launch reads A from A + a_offset and B from B + b_offset (elements); C is
 * uploaded first, so what the kernel does not write keeps its value.  route_out[4] = {route (tgemm.h TgRouteKind), avec,
 * bvec, acc64}, written before the launch (also when it is refused); flops_out = the launch's flop counter. */
int pepsgpu_diag_tgemm_desc(int types, const int *desc_ints, int n_ints, const long *desc_longs, int n_longs,
                            const double *desc_dbls, int n_dbls, const int32_t *pool, long pool_n, const float *scale_in,
                            const void *A, size_t a_elems, long a_offset, const void *B, size_t b_elems, long b_offset,
                            void *C, size_t c_elems, float *scale_out, double *norm_log, int32_t *norm_flag,
                            int32_t *route_out, unsigned long long *flops_out);
/* the route tgemm_launch would take for the same descriptor, without a device (operands at a 256-byte aligned base
 * advanced by the offsets) */
int pepsgpu_diag_tgemm_route(int types, const int *desc_ints, int n_ints, const long *desc_longs, int n_longs,
                             const double *desc_dbls, int n_dbls, long a_offset, long b_offset, int32_t *route_out);
/* one BTen growth step through tgemm_chain3_kernel with the descriptors of the engine's bten_step; see capi.hip */
int pepsgpu_diag_tgemm_chain3(const int *dims8, const int *site_strides4, long slot, int nslots, const int32_t *sel, int sel_inc,
                              const int32_t *live4, const int32_t *skip, int nbatch, const int *offs3, const float *mps1,
                              const float *bten, const float *site, const float *mps2, float *out, int32_t *flags_out,
                              int32_t *launched_out, int32_t *variant_out);
/* trace_dot4_kernel alone (the closure of the two-row traces): out[b] = exp(lsum[b]) sum_{ijkl} a[b][i][j][k][l] b[b][l][k][j][i] for
 * nbatch entries of dims4 = (I, J, K, L), no conjugation, float64 / complex float64 accumulation; dtype PEPSGPU_F32 / F64 / C128 (out
 * then holds interleaved pairs).  flag (may be NULL, the batch_flag convention of the tensor GEMM): an entry with flag[b] >= 0 is
 * skipped and writes 0.0. */
int pepsgpu_diag_dot4(int dtype, const void *a, const void *b, const int *dims4, int nbatch, const double *lsum, const int32_t *flag,
                      double *out);
int pepsgpu_diag_chol(int dtype_out, const double *G, int n, int nbatch, void *R_out);
/* the streaming f64 Gram kernel of the forward pass (gram.h): P = [nbatch][K][n], klive (nullable) = live rows per entry */
int pepsgpu_diag_gram_cols(int dtype, const void *P, int K, int n, int nbatch, const int32_t *klive, double *G_out);
int pepsgpu_diag_gram_rows(const float *M, int n, int K, int nbatch, const int32_t *nrows, double *G_out);
int pepsgpu_diag_mgemm_dense(const float *R, const float *Tt, int m, int la, int a_dim, int u_dim, int k2_dim, int tt_u_inner, int nbatch,
                             const int32_t *m_live, const int32_t *a_live, const int32_t *k2_live, float *M_out);
/* diagnostics (PEPSGPU_CG_STATS=1): per-phase counters of colgram_dense_kernel, read and reset; see trunc_mid.h */
int pepsgpu_diag_cg_stats(double *out16);
/* the LDS-resident Gram + Cholesky kernels alone (f32): which = 0 rows form (X = [nbatch][n][K], R^T R = X X^T, nlive = live rows),
 * which = 1 column form (X = [nbatch][K][n], R^T R = X^T X, nlive = live rows of X); R_out = [nbatch][n][n], n <= 128 */
int pepsgpu_diag_lds_gram_chol(int which, const float *X, int n, int K, int nbatch, const int32_t *nlive, float *R_out, int32_t *mlive_out);
/* the first compression of the dense truncation route as it runs (round 6): i8 row Gram with both triangles + the diagonally pivoted
 * factorisation stopped after kcap <= 64 rows (chol_pivot.h); X = [nbatch][n][K] f32, 128 < n <= 256; R_out = [nbatch][kcap][n], rows in pivot order */
int pepsgpu_diag_chol_pivot(const float *X, int n, int K, int nbatch, const int32_t *nlive, int kcap, float *R_out, int32_t *mlive_out);
/* rows_qr_kernel alone (round 6): the k <= 32 nearly orthogonal rows X = [nbatch][k][len] (len <= 256, by decreasing norm) made orthonormal in
 * float64 (Cholesky-QR of the unit-scaled rows); V_out: live rows first, the rest zero; klive_out = their count */
int pepsgpu_diag_rows_qr(const float *X, int k, int len, int nbatch, const int32_t *klive, float *V_out, int32_t *klive_out);
/* the device's SuwaTodoStateUpdate alone (round 6, the decision of pepsgpu_sweep_slice_fullspace): a chain of `steps` updates on one
 * weight vector (n <= 16), words = 2 * steps raw outputs of the caller's std::mt19937; out_chain[s] = the state after step s */
int pepsgpu_diag_suwa_todo(const double *weights, int n, int init, const uint32_t *words, int steps, int32_t *out_chain);
/* the rank-adaptive pair used by the absorption: low-rank right-looking kernel, then the blocked
 * kernel for the walkers whose rank exceeds its cap; mlive_out[b] = rows of R_out[b] that exist */
/* the Gram-free low-rank kernel alone: P = [nbatch][K][n] (dtype), R^T R = P^T P; mlive_out[b] = -1 where
 * it declines (K or the rank above its caps) and the Gram + Cholesky pair has to run */
/* forward contraction pair of an absorption through the LDS-chained kernel (tgemm_chain_kernel); see capi.hip */
int pepsgpu_diag_tgemm_chain(const int *dims7, const int32_t *live3_per_entry, int nbatch, const float *R, const float *A,
                             const float *W, float *P_out, int32_t *flags_out);
/* the forward pair (backward = 0: P = W (R A)) or the backward pair (1: Tt = W (A Y)) of an absorption with the engine's descriptors,
 * the site tensor reached through a selector table; opts & 1 asks for the leg-8 kernel (tgemm_d8.h) where its shape contract holds,
 * else tgemm_chain_kernel runs; info_out = {launcher's return, 1 when the leg-8 kernel ran}; see capi.hip */
int pepsgpu_diag_tgemm_chain_pair(int backward, const int *dims8, const int *site_strides4, long slot, int nslots, const int32_t *sel,
                                  const int32_t *live3_per_entry, int nbatch, int opts, const float *scale_in, const float *op1,
                                  const float *op2, const float *site, float *out, int32_t *flags_out, int32_t *info_out);
/* launches of the leg-8 chained-pair kernel by this process (PEPSGPU_CHAIN_D8=0 keeps it at zero) */
long pepsgpu_diag_chain_d8_launches(void);
/* PEPSGPU_CHAIN_D8_STATS=1: out2 = {walkers the leg-8 kernel computed, of them walked in chunks of the intermediate}; else zeros */
int pepsgpu_diag_chain_d8_stats(unsigned long long *out2);
int pepsgpu_diag_gram_chol(int dtype, const void *P, int K, int n, int nbatch, void *R_out, int32_t *mlive_out);
/* one of the two one-wave Gram-free factor kernels alone, launched as the engine launches it (form 0: gram_chol_wave_kernel, four
 * walkers per 256-thread block; 1: gram_chol_wave_split_kernel, the row-parity placement, one walker per 64-thread block), then the
 * list kernel for the walkers it hands on: P = [nbatch][K][n] float32, klive[b] live rows,
 * columns (outer, inner) with inner_live[b] live inner indices (NULL: all); R_out [nbatch][n][n] is read as well: what no
 * kernel stores comes back unchanged */
int pepsgpu_diag_gram_chol_wave(const float *P, int K, int n, int nbatch, const int32_t *klive, int inner,
                                const int32_t *inner_live, int max_pass, int form, float *R_out, int32_t *mlive_out);
int pepsgpu_diag_chol_adaptive(int dtype_out, const double *G, int n, int nbatch, void *R_out, int32_t *mlive_out);
/* dtype PEPSGPU_C128: the general complex Jacobi (jacobi_rows_cplx_kernel, at most 60 sweeps) and the select; M and Vt_out are
 * interleaved (re, im), S_out [nbatch][k] stays real float64, force_global is ignored */
int pepsgpu_diag_jacobi(int dtype, void *M, int m, int len, int nbatch, int k, void *Vt_out, void *S_out,
                        int force_global, int *sweeps_out);
/* The pieces only the float64 / complex dense truncation routes launch, one launch each; element type float64, or (is_complex != 0)
 * interleaved complex float64.
 * pepsgpu_diag_chol_solve_rows: one Cholesky-QR pass X <- L^-1 X, L L^H = S.  S = [nbatch][64][64], upper triangle read; X =
 *   [nbatch][r_max][len] in place, r_max <= 64.  float64: rows[b] <= r_max rows of entry b; complex: r rows of every entry (rows
 *   ignored).  run_flag (nullable): entries with run_flag[b] >= 0 are left alone.
 * pepsgpu_diag_gather_rows: Q[b][j][:] = M[b][piv[b][j]][:] for j < rows[b] (<= min(slots, 64)) where piv >= 0; M = [nbatch][m][len],
 *   piv = [nbatch][slots], Q = [nbatch][64][len] is read as well: what the kernel leaves comes back unchanged.
 * pepsgpu_diag_sign_table: the fixed table of +1 / -1 the complex range finder starts from, out = [rows][cols].
 * pepsgpu_diag_truncate_site: the truncation of ONE interior site of a PEPSGPU_F64 or PEPSGPU_C128 context as a row absorption runs
 *   it, on nbatch <= max_walkers given matrices M = [nbatch][m][u * k2]; k = min(chi_max, m, u * k2).  rows (float64 only, nullable):
 *   live rows of M per entry.  route: 0 = the dispatch as shipped (PEPSGPU_F64_PIVOT, PEPSGPU_NO_F64_DENSE_ROUTE,
 *   PEPSGPU_NO_C128_DENSE_ROUTE as the process read them), 1 = the round-6 form (pivoted rows / range finder), 2 = the round-5
 *   two-Cholesky form (blocks of more than 128 rows and no more rows than columns; others: general kernels), 3 = general kernels only; 1 .. 3 override the environment for this call.  V_out = [nbatch][k][u * k2];
 *   klive_out [nbatch] = live rows of V (-1 on a complex context, which keeps static shapes); route_flag_out [nbatch]: < 0 = a dense
 *   route delivered the entry's rows, >= 0 = the general kernels did.  The context's walkers and environments are not touched. */
int pepsgpu_diag_chol_solve_rows(int is_complex, const void *S, void *X, int nbatch, int r_max, int len, const int32_t *rows, int r,
                                 const int32_t *run_flag);
int pepsgpu_diag_gather_rows(int is_complex, const void *M, int nbatch, int m, int len, const int32_t *piv, int slots,
                             const int32_t *rows, const int32_t *run_flag, void *Q);
int pepsgpu_diag_sign_table(int is_complex, int rows, int cols, void *out);
int pepsgpu_diag_truncate_site(pepsgpu_ctx *ctx, const void *M, int nbatch, int m, int u, int k2, const int32_t *rows, int route,
                               void *V_out, int32_t *klive_out, int32_t *route_flag_out);
/* the short-row Jacobi with its select epilogue alone (jacobi_rows_tiny4_kernel, the form the low-rank sites launch):
 * M = [nbatch][m][len] float32 (len <= 128, not written), rows[b] live rows of entry b, k rows of Vt per entry, span != 0 asks for
 * the span path (JrSelect::span).  Vt_out [nbatch][k][len], klive_out and sweeps_out [nbatch] are read as well: an entry
 * the kernel does not take (0 or more than 16 live rows) comes back unchanged.  sweeps word: sweeps | live rows << 8 */
int pepsgpu_diag_trunc_rows(const float *M, int m, int len, int nbatch, const int32_t *rows, int k, int span, float *Vt_out,
                            int32_t *klive_out, int32_t *sweeps_out);
const char *pepsgpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PEPSGPU_H */
