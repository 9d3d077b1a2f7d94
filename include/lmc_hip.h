/*
 * lmc_hip.h -- C ABI of the MI355X-native many-chain HMC/NUTS engine (liblmc_hip.so).
 *
 * This is the drop-in boundary for the hot path of eigenfoo/littlemcmc 0.2.2. The reference has
 * no FFI: its boundary is a set of duck-typed Python contracts. Each entry
 * point below names the reference interface it replaces (paths relative to
 * /root/reference/littlemcmc/); the Python mirror in littlemcmc_amd/ binds them with ctypes
 * (see INTEGRATION.md for the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - plain C: opaque handle, pointers + sizes, int status returns (0 = LMC_OK); no C++ exceptions
 *     and no torch types cross this boundary;
 *   - array arguments may be HOST or DEVICE pointers (copies use hipMemcpyDefault); shapes are
 *     row-major and UNPADDED: positions [chains][dim], per-chain scalars [chains];
 *   - one engine == one GPU == one HIP stream; a handle is not thread-safe;
 *   - all work is enqueued on the engine's stream; calls that return data synchronise it;
 *   - per-chain numerical failures are reported through status bits, never by aborting the launch.
 */
#ifndef LMC_HIP_H_
#define LMC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMC_ABI_VERSION 9

/* status codes */
#define LMC_OK 0
#define LMC_ERR_INVALID 1      /* bad argument / unsupported configuration */
#define LMC_ERR_HIP 2          /* a HIP runtime call failed; see lmc_last_error() */
#define LMC_ERR_STATE 3        /* call sequence error (e.g. run before reserve) */

/* step method: nuts.py:32 (NUTS) / hmc.py:30 (HamiltonianMC) */
#define LMC_KIND_NUTS 0
#define LMC_KIND_HMC 1

/* mass matrix: quadpotential.py:148 (QuadPotentialDiagAdapt, float32 momentum draw, adapted during
 * tuning) / quadpotential.py:346 (QuadPotentialDiag, fixed diagonal, float64 momentum draw) */
#define LMC_POT_DIAG_ADAPT 0
#define LMC_POT_DIAG 1
/* dense mass matrices ("Which kernels an engine runs" below for the sizes): quadpotential.py:428 (QuadPotentialFull: float32 covariance, float32
 * momentum by a triangular solve), :388 (QuadPotentialFullInv: mass matrix A given, float64 momentum L n),
 * :471 (QuadPotentialFullAdapt: covariance + Cholesky factor re-estimated while tuning, one matrix per chain) */
#define LMC_POT_FULL 2
#define LMC_POT_FULL_INV 3
#define LMC_POT_FULL_ADAPT 4
/* QuadPotentialFull(cov, dtype="float64") (quadpotential.py:431-444, the dtype argument): float64 covariance, float64
 * velocity (dgemv), float64 momentum solve_triangular(chol.T, float64 normals). Same kernels as FULL_INV (float64 matrix
 * sweeps); the momentum is the sweep of L^-1, formed once on the host in extended precision. */
#define LMC_POT_FULL_F64 5

/* built-in device log-densities (littlemcmc_amd/csrc/lmc_targets.hpp); LMC_TARGET_USER exists only in
 * libraries built with a user target header (littlemcmc_amd/targets.py: UserTarget) */
#define LMC_TARGET_STD_NORMAL 0
#define LMC_TARGET_DIAG_GAUSSIAN 1   /* params: prec[dim] */
#define LMC_TARGET_AR1 2             /* params: {c_end, c_mid, off} */
#define LMC_TARGET_FUNNEL 3
#define LMC_TARGET_NORMAL1D 4        /* params: {loc, scale}; dim must be 1 */
#define LMC_TARGET_USER 5
/* no device functor: the caller evaluates logp_dlogp_func for all chains between two lmc_engine_tick() calls
 * (a batched callable on device memory, e.g. torch-ROCm); all potentials (dense ones up to dim 256) */
#define LMC_TARGET_EXTERNAL 6
/* Generalised linear model that carries its data (additive within ABI 9; littlemcmc_amd/targets.py: GLM). Coefficients q[dim],
 * design matrix X[N][dim], responses y[N], linear predictor eta = X q, prior q_e ~ N(0, 1/tau); constants that do not depend
 * on q are dropped:
 *   logp = sum_n l_n - 1/2 tau sum_e q_e^2,   g_e = sum_n X[n][e] r_n - tau q_e
 *   LMC_GLM_BERNOULLI (logit link, y in {0, 1}):  l = y eta - softplus(eta),       r = y - sigmoid(eta)
 *   LMC_GLM_POISSON   (log link, y >= 0):         l = y eta - exp(eta),            r = y - exp(eta)
 *   LMC_GLM_GAUSSIAN  (identity, known sigma):    l = -1/2 (y - eta)^2 isig2,      r = (y - eta) isig2
 * One chain is one wavefront: dim <= LMC_GLM_MAX_DIM, refused beyond. The parameter row is doubles only. With
 * npad = N rounded up to a multiple of 64, d8 = dim rounded up to a multiple of 8 and dpad = 64 * (dim / 64 rounded up to a
 * power of two: the lanes of the chain's wavefront times the elements each of them owns):
 *   [0] likelihood code  [1] N  [2] npad  [3] tau = prior_scale^-2  [4] isig2 = sigma^-2  [5] dim  [6] dpad  [7] 0
 *   [8, 8 + npad)                      y[n]
 *   [8 + npad, +d8 * npad)             Xt[e][n] = X[n][e], row e at stride npad   (the eta pass: lane = observation)
 *   [8 + npad * (1 + d8), +npad*dpad)  Xr[n][e] = X[n][e], row n at stride dpad   (the gradient pass: lane = coefficients)
 * That is 8 + npad * (1 + d8 + dpad) doubles in all, below LMC_GLM_MAX_ROW (the device addresses a row with 32-bit byte
 * offsets). Everything beyond n = N or e = dim is zero; every section starts 16-byte aligned (all offsets are even). The
 * setters refuse (LMC_ERR_INVALID, before any HIP call) a row whose length is not the one its header and the engine's dim give,
 * a header that does not match the engine's dim, and an unknown likelihood code; lmc_target_groups_check(), which sees no
 * table, refuses a length that no N gives at that dim. X and y are finite (the padding rows of Xt are multiplied by the
 * zero padding coefficients, not skipped). */
/* (7 stays unassigned: lmc_has_target(7) is 0) */
#define LMC_TARGET_GLM 8
#define LMC_GLM_BERNOULLI 0
#define LMC_GLM_POISSON 1
#define LMC_GLM_GAUSSIAN 2
#define LMC_GLM_MAX_DIM 512
#define LMC_GLM_HEADER 8
#define LMC_GLM_MAX_ROW (1LL << 29)

/* Summation order of the float32 kinetic energy of the start state, 0.5f * sdot(p, v)
 * (integration.py:63-64 with float32 operands -> numpy -> OpenBLAS cblas_sdot). The value feeds the
 * accept statistic and, through dual averaging, every later step size, so same-seed parity beyond
 * ~1e-6 needs the host BLAS's rounding. NATIVE: exact products summed in float64, rounded once. */
#define LMC_SDOT_NATIVE 0
#define LMC_SDOT_OPENBLAS_SKYLAKEX 1   /* OpenBLAS 0.3.29 sdot_k_SKYLAKEX (AVX-512 hosts); default */
#define LMC_SDOT_OPENBLAS_HASWELL 2    /* OpenBLAS 0.3.29 sdot_k_HASWELL (AVX2 hosts) */

/* Where the momentum draw's normals come from (potential.random(), quadpotential.py:221-224 / :374-376).
 * NUMPY: the reference's own stream -- per-chain legacy MT19937 + polar method in numpy's consumption order (same-seed
 * parity; the default). PHILOX: a counter-based stream, Philox4x32-10 keyed by the chain's seed and counted by
 * (iteration, element), float32 Box-Muller: the throughput mode for callers that do not need the reference's draws
 * (the momentum draw is ~20 % of a depth-3 iteration on the parity stream). Tree uniforms stay on MT19937 in both.
 * Fused diagonal-mass kernels with the built-in densities (in a team of wavefronts every thread draws its own
 * elements: the draw needs no barrier, where the parity stream is produced by wave 0 alone).
 * COUNTER: PHILOX's momentum draw, and every uniform of the transition -- the device step jitter's, the tree's directions
 * and merges, HMC's path length and acceptance -- from a second counter-based stream: u_k, the k-th uniform iteration
 * `git` of a chain consumes (k from 0 in the sequential algorithm's order), is
 *   w = philox4x32_10(c0 = (uint32)git, c1 = (uint32)(git >> 32), c2 = k >> 1, c3 = 0x6c6d6375 "lmcu", k0 = seed, k1 = 0x4d4f4d31)
 *   (a, b) = (w[0], w[1]) for even k, (w[2], w[3]) for odd k;   u_k = ((a >> 5) * 2^26 + (b >> 6)) / 2^53   in [0, 1)
 * (the momentum stream counts (git, thread) under c3 = 0x6c6d636d "lmcm": disjoint counter spaces). What iteration t of a
 * chain does is then a pure function of (seed, t, the chain's state): no generator state exists -- the chain's MT19937
 * arrays are neither read nor written, the kernels reserve no LDS for them -- results do not depend on launch slicing or
 * on the chain-block partition, and lmc_engine_counter_draws() hands out the very numbers, so that a host model replays
 * any iteration. Fused diagonal-mass kernels with the built-in densities AND run-time compiled user densities
 * (LMC_TARGET_USER); refused (LMC_ERR_INVALID) with dense mass matrices, in the general kernels and with
 * LMC_TARGET_EXTERNAL. Not same-seed comparable with the reference, nor with PHILOX. */
#define LMC_RNG_NUMPY 0
#define LMC_RNG_PHILOX 1
#define LMC_RNG_COUNTER 2

/* LDS plan of the one-wave fused sampling kernels (csrc/lmc_sampler.hpp: PairLds<NS, 1, PL>). SHALLOW keeps the chain's
 * MT19937 state and the cold slots of the trajectory in LDS and subtree-stack level 1; DEEP uses the generator in place
 * (HBM/L2), one cold slot, and the room that frees holds stack level 2 -- faster once trees are deep (C3: +6 %). AUTO (the
 * default): the engine picks the plan of every launch when it is enqueued, from the mean tree size the running chains report
 * (plan SHALLOW for launches that start before iteration 200). Same statements, same results bit for bit under either plan
 * (tests/test_gpu_round5.py); the pinned values exist for A/B runs and for putting either kernel under the oracle. Ignored
 * by team (dim > 256), dense, general and tick kernels. */
#define LMC_LDS_PLAN_AUTO 0
#define LMC_LDS_PLAN_SHALLOW 1
#define LMC_LDS_PLAN_DEEP 2

/* per-chain status bits (lmc_engine_get_status) */
#define LMC_STATUS_BAD_INITIAL_ENERGY 1   /* base_hmc.py:145-148 (ValueError in the reference) */
/* (No bit for math.py:23-24's FloatingPointError: logbern() only sees log-weights of leaves that passed the divergence
 * test |dE| < Emax (nuts.py:358; a NaN dE becomes +inf first, and inf < Emax is false even for Emax = inf), so every
 * log_size entering a merge is finite and log_p cannot be NaN -- the error is unreachable through this path.) */

/* per-draw statistics. f64 slots */
#define LMC_STAT_STEP_SIZE 0        /* "step_size": exp(log_step) after the update (step_sizes.py:94-99) */
#define LMC_STAT_STEP_SIZE_BAR 1    /* "step_size_bar" */
#define LMC_STAT_ACCEPT 2           /* NUTS "mean_tree_accept" (nuts.py:421-425) / HMC "accept" (hmc.py:164) */
#define LMC_STAT_ENERGY_ERROR 3     /* "energy_error" */
#define LMC_STAT_ENERGY 4           /* "energy" */
#define LMC_STAT_MAX_ENERGY_ERROR 5 /* NUTS "max_energy_error" / HMC "path_length" */
#define LMC_STAT_MODEL_LOGP 6       /* "model_logp" */
#define LMC_NUM_STAT_F64 7
/* i32 slots */
#define LMC_STAT_DEPTH 0            /* NUTS "depth" / HMC "n_steps" */
#define LMC_STAT_TREE_SIZE 1        /* NUTS "tree_size" (= leapfrog steps, nuts.py:432) / HMC n_steps */
#define LMC_NUM_STAT_I32 2
/* u8 slots */
#define LMC_STAT_DIVERGING 0        /* "diverging" */
#define LMC_STAT_TUNE 1             /* "tune" */
#define LMC_STAT_ACCEPTED 2         /* HMC "accepted" */
#define LMC_NUM_STAT_U8 3

/* per-chain counters (lmc_engine_get_counters), int64 [chains][LMC_NUM_COUNTERS] */
#define LMC_CT_REACHED_MAX_TREEDEPTH 0   /* nuts.py:218-220 */
#define LMC_CT_DIVS_AFTER_TUNE 1         /* base_hmc.py:171 */
#define LMC_CT_SAMPLES_AFTER_TUNE 2      /* base_hmc.py:183 */
#define LMC_CT_LEAPFROGS 3               /* sum of tree_size / n_steps: the bench metric's numerator */
#define LMC_CT_WAVE_TICKS 4              /* wall-clock ticks (lmc_engine_occupancy: wall_clock_hz) the chain's wavefronts were
                                          * resident in lmc_engine_run() launches: sum over chains / (resident slots x launch
                                          * time) = mean wave-slot occupancy; the reference's analogue is a chain's process
                                          * time (parallel_sampling.py:377-496). Fused diagonal-mass kernels only. */
#define LMC_NUM_COUNTERS 5

typedef struct lmc_engine lmc_engine;

/* Kernel-selection and layout knobs, every one 0 = the engine decides. They exist for tests (replaying the small goldens
 * through the general kernels, the large team, the HBM factorisation) and for A/B measurements; a result never depends on
 * them beyond the tolerance the selected kernel documents. Until ABI 7 these were environment variables read inside the
 * library -- hidden inputs to an ABI that takes everything else through lmc_config; the Python host still honours the
 * variables of the same names (littlemcmc_amd/engine.py: tuning_from_env), but it is the host that reads them. */
typedef struct lmc_tuning {
    int32_t sub_blocks;           /* sub-block streams lmc_engine_run() deals the chains to: 1 .. 4 (LMC_SUB_BLOCKS); -n: at most n */
    int32_t force_general;        /* 1: every shape the general kernels support runs in them (LMC_FORCE_WIDE) */
    int32_t general_team;         /* 16: the general kernels' 16-wavefront team at every shape (LMC_WIDE_TEAM) */
    int32_t run_ns, run_w;        /* shape of the fused sampling kernel, 64 * run_ns * run_w = padded dim (LMC_RUN_SHAPE="ns,w") */
    int32_t dense_coop_off;       /* 1: QuadPotentialFull never takes the cooperative shared-matrix kernel (LMC_DENSE_COOP=0) */
    int32_t dense_cache_rows_p1;  /* rows of the matrix a dense kernel caches in LDS, PLUS ONE (LMC_DENSE_CACHE_ROWS) */
    int32_t dense_lds_slots_p1;   /* leading tree slots a dense kernel keeps in LDS, PLUS ONE (LMC_DENSE_LDS_SLOTS) */
    int32_t chol_hbm;             /* 1: FullAdapt's refresh factorises through HBM at every size (LMC_CHOL_HBM) */
    int32_t leaf_group;           /* NUTS tree build of the one-wave sampling kernels of <= 2 elements per lane: 2 = leaf pairs,
                                   * 4 = leaf quads (the default), 0 = the engine decides; other shapes always build from pairs.
                                   * Results do not depend on it (LMC_LEAF_GROUP) */
    int32_t reserved[2];          /* must be 0 */
} lmc_tuning;

/* Constructor arguments of the step method: BaseHMC.__init__ (base_hmc.py:32-126) +
 * NUTS.__init__ (nuts.py:103-202) + HamiltonianMC.__init__ (hmc.py:52-138). */
typedef struct lmc_config {
    int32_t abi_version;          /* LMC_ABI_VERSION */
    int32_t device;               /* HIP device ordinal */
    int32_t chains;               /* chains owned by this engine (one wavefront each) */
    int32_t dim;                  /* model_ndim */
    int32_t kind;                 /* LMC_KIND_* */
    int32_t target_family;        /* LMC_TARGET_* */
    int32_t potential;            /* LMC_POT_* */
    int32_t adapt_step_size;      /* bool */
    double target_accept;         /* 0.8 */
    double emax;                  /* 1000 */
    double step_scale;            /* 0.25; initial step = step_scale / dim**0.25 (base_hmc.py:102) */
    double gamma;                 /* 0.05 */
    double k;                     /* 0.75 */
    double t0;                    /* 10 */
    int32_t max_treedepth;        /* 10 */
    int32_t early_max_treedepth;  /* 8 */
    double path_length;           /* 2.0 (HMC) */
    int32_t max_steps;            /* 1024 (HMC) */
    int32_t adaptation_window;    /* 101 (quadpotential.py:156) */
    int32_t lds_levels;           /* subtree-stack levels kept in LDS; 0 = choose automatically */
    int32_t start_energy_sdot;    /* LMC_SDOT_*: summation order of the float32 start-state kinetic energy */
    double adaptation_window_multiplier; /* 1.0: QuadPotentialDiagAdapt's window grows by this factor at every switch (quadpotential.py:243) */
    int32_t rng_mode;             /* LMC_RNG_*; 0 = the reference's stream */
    int32_t mass_f64;             /* QuadPotentialDiagAdapt(dtype="float64") (quadpotential.py:159,175-184): variance, standard deviations
                                   * and the momentum draw stay float64; with LMC_POT_FULL_ADAPT: QuadPotentialFullAdapt(dtype="float64")
                                   * (:484,497-509): float64 covariance, Cholesky factor and momentum solve. 0 = the reference's
                                   * default float32. General kernels (below). */
    int32_t lds_plan;             /* LMC_LDS_PLAN_*: which LDS plan the one-wave sampling kernels run under (results do not
                                   * depend on it). 0 = the engine chooses per launch. */
    int32_t reserved0;            /* must be 0 */
    lmc_tuning tuning;            /* all zero = the engine decides */
} lmc_config;

/* Which kernels an engine runs. The FUSED kernels (one chain = one wavefront or a team of 2 / 4, the tree in registers and
 * LDS) cover dim <= 1024 with diagonal and dim <= 256 with dense mass matrices, float32 adaptive masses. Everything else the
 * reference accepts -- dim up to 16 384 (base_hmc.py:102 has no limit), QuadPotentialFull / FullInv up to dim 2048
 * (quadpotential.py:388-468), QuadPotentialFullAdapt up to dim 1024 (:470-560; the refresh then factorises through HBM),
 * QuadPotentialDiagAdapt / QuadPotentialFullAdapt(dtype="float64") -- runs in the GENERAL kernels (csrc/lmc_wide.hpp: one
 * chain = one wavefront up to dim 512, a workgroup of 16 wavefronts beyond, the tree in the chain's HBM row): the same
 * algorithm, statement for statement, several times slower per leapfrog. Not in the general kernels: LMC_RNG_PHILOX / LMC_RNG_COUNTER, and LMC_TARGET_EXTERNAL with
 * anything but a float32 diagonal. A shared matrix adapted from all chains (lmc_engine_pool_*, LMC_POT_FULL up to dim 256) samples
 * in the LMC_POT_FULL kernels; its statistic is formed by pool_accumulate_kernel (csrc/lmc_pool.hip) on the matrix cores. */
/* Fill *cfg with the reference's defaults for the given shape. */
void lmc_config_defaults(lmc_config* cfg, int32_t chains, int32_t dim);

/* Library-wide: message of the last failure on this thread (engine may be NULL). */
const char* lmc_last_error(const lmc_engine* e);
int32_t lmc_abi_version(void);
/* Identity of THIS binary: the hash of the sources, header and compiler flags it was compiled from
 * (littlemcmc_amd/_build.py: source_hash(), passed as -DLMC_SOURCE_HASH at build time; "unstamped" for a build made
 * any other way). Measurements under profiles/ are only quoted for the binary whose hash they carry. */
const char* lmc_build_hash(void);
/* HIP devices visible to this process (0: none, or no usable HIP runtime). One engine runs on one of them
 * (lmc_config.device); a job on several is one engine per device on a contiguous chain block each -- the reference's
 * `cores` (sampling.py:117-129) with GPUs in the place of worker processes. */
int32_t lmc_device_count(void);
/* 1 if this library was built with the given LMC_TARGET_* family. */
int32_t lmc_has_target(int32_t family);

/* ---- lifecycle: NUTS(...) / HamiltonianMC(...) construction ------------------------------------ */
int lmc_engine_create(const lmc_config* cfg, lmc_engine** out);
void lmc_engine_destroy(lmc_engine* e);
/* Launch on an externally owned hipStream_t (e.g. torch's current stream). NULL = engine's own. On an external stream
 * every lmc_engine_run() is ordered after whatever the caller enqueued on that stream before the call, and the stream is
 * ordered after the run's kernels on return (event waits on the device): the caller's own work on the stream needs no
 * lmc_engine_synchronize(). (With the engine's own stream consecutive runs overlap per sub-block instead.) */
int lmc_engine_set_stream(lmc_engine* e, void* hip_stream);
int lmc_engine_synchronize(lmc_engine* e);

/* ---- plug-in parameters: the closure of the user's logp_dlogp_func (integration.py:40) ----------- */
int lmc_engine_set_target_params(lmc_engine* e, const double* params, int64_t n);
/* Per-group parameters (additive within ABI 9): many posteriors in one job. `params` is a host table [n_groups][n_per_group],
 * row-major; chain j of the JOB evaluates the density on row j / chains_per_group, and this engine's chain c is chain
 * first_chain + c of the job (an engine holds one contiguous block of a job's chains; the block may begin and end inside a
 * group). The kernels choose the row once per launch, where they call the functor's init(Team&, const double* params, int d):
 * no functor changes, a run-time compiled one included, and chain c computes bit for bit what it computes in an engine
 * whose lmc_engine_set_target_params() got that row. On the device the rows start 16-byte aligned (the distance between rows
 * is n_per_group rounded up to an even number of doubles, the pad is zero).
 * Refused with LMC_ERR_INVALID before any HIP call: n_groups < 1, chains_per_group < 1, first_chain < 0, n_per_group < 0,
 * a row length the family does not take (as lmc_engine_set_target_params: diag_gaussian dim, ar1 3, normal1d 2), and a
 * table too short for the engine's chains: (first_chain + chains - 1) / chains_per_group >= n_groups.
 * lmc_engine_set_target_params() is the case of one row for all chains; calling it again returns the engine to that.
 * lmc_engine_target_groups(): what the engine holds (NULL pointers are skipped); an engine without a table reports
 * n_groups 1, n_per_group n, first_chain 0, chains_per_group chains. */
int lmc_engine_set_target_params_grouped(lmc_engine* e, const double* params, int64_t n_groups, int64_t n_per_group,
                                         int64_t first_chain, int64_t chains_per_group);
int lmc_engine_target_groups(lmc_engine* e, int64_t* n_groups, int64_t* n_per_group, int64_t* first_chain, int64_t* chains_per_group);
/* The row arithmetic as a pure function (no engine, no GPU): *row = (first_chain + chain) / chains_per_group for chain `chain`
 * of an engine whose chain 0 is the job's chain first_chain. chain, first_chain in [0, 2^31), chains_per_group in [1, 2^31),
 * else LMC_ERR_INVALID. */
int lmc_target_param_row(int64_t chain, int64_t first_chain, int64_t chains_per_group, int64_t* row);
/* Everything lmc_engine_set_target_params_grouped() refuses, for an engine of `chains` chains of dimension `dim` and family
 * `target_family`, as a pure function (no engine, no GPU): the setter calls exactly this before its first HIP call. */
int lmc_target_groups_check(int32_t target_family, int32_t dim, int32_t chains, int64_t n_groups, int64_t n_per_group,
                            int64_t first_chain, int64_t chains_per_group);

/* ---- potential: QuadPotentialDiagAdapt(n, initial_mean, initial_diag, initial_weight)
 *      (quadpotential.py:151-204) or QuadPotentialDiag(v) (quadpotential.py:349-365).
 *      initial_mean / initial_diag: [dim] (per_chain = 0, shared) or [chains][dim].
 *      Also performs reset(). initial_mean may be NULL for LMC_POT_DIAG. */
int lmc_engine_set_potential(lmc_engine* e, const double* initial_mean, const double* initial_diag,
                             double initial_weight, int32_t per_chain);

/* ---- dense potentials (cfg.potential = LMC_POT_FULL / FULL_INV / FULL_ADAPT). matrix: [dim][dim] row-major,
 *      the same for every chain.
 *      FULL:       QuadPotentialFull(cov) (quadpotential.py:431-444): matrix = covariance, cast to float32 and
 *                  factorised (failure -> LMC_ERR_INVALID, as scipy.linalg.cholesky raises).
 *      FULL_INV:   QuadPotentialFullInv(A) (quadpotential.py:391-402): matrix = A (inverse covariance).
 *      FULL_F64:   QuadPotentialFull(cov, dtype="float64"): matrix = covariance, kept in float64.
 *      FULL_ADAPT: QuadPotentialFullAdapt(n, initial_mean, initial_cov, initial_weight, adaptation_window,
 *                  adaptation_window_multiplier, update_window) (quadpotential.py:474-519); matrix = initial_cov.
 *      initial_mean .. update_window are read for FULL_ADAPT only. Also the state reset_tuning() restores. */
int lmc_engine_set_dense_potential(lmc_engine* e, const double* matrix, const double* initial_mean,
                                   double initial_weight, int32_t adaptation_window,
                                   double adaptation_window_multiplier, int32_t update_window);

/* ---- RNG: np.random.seed(seeds[c]) for every chain (sampling.py:496-497) ------------------------- */
int lmc_engine_seed(lmc_engine* e, const uint32_t* seeds);
/* np.random.get_state()/set_state() of one chain: key[624], pos, has_gauss, cached_gaussian */
int lmc_engine_set_rng_state(lmc_engine* e, int32_t chain, const uint32_t* key, int32_t pos,
                             int32_t has_gauss, double gauss);
int lmc_engine_get_rng_state(lmc_engine* e, int32_t chain, uint32_t* key, int32_t* pos,
                             int32_t* has_gauss, double* gauss);

/* ---- positions: the `q` threaded through step._astep(q) (sampling.py:498,512) ------------------- */
int lmc_engine_set_position(lmc_engine* e, const double* q, int32_t per_chain);
int lmc_engine_get_position(lmc_engine* e, double* q);

/* ---- tuning lifecycle: step.reset_tuning() + iter_count = 0 (base_hmc.py:192-200, sampling.py:503-509) */
int lmc_engine_reset_tuning(lmc_engine* e);
/* Overwrite the dual-averaging state of every chain (step_sizes.py:49-56 fields). */
int lmc_engine_set_dual_average(lmc_engine* e, double log_step, double log_bar, double hbar,
                                int32_t count);

/* ---- sampling: the body of _iter_sample (sampling.py:507-521) for ALL chains ---------------------
 * reserve(): allocate output storage for `capacity` iterations per chain. Draws are stored for iterations
 *        >= trace_begin (0 = all, tune = discard_tuned_samples, < 0 = keep no trace: statistics only).
 * run(): iterations [iter_begin, iter_begin + n_iters) of every chain; iterations with global index
 *        < n_tune are tuning iterations (stop_tuning happens at index n_tune, sampling.py:510-511).
 *        Asynchronous. Chains are independent (sampling.py:131-136: one process per chain in the reference), so
 *        the engine launches them as contiguous sub-blocks on internal streams of their own (FOUR for the fused diagonal-mass
 *        kernels, two for the dense ones, one for the general kernels; lmc_engine_run_streams() returns the number --
 *        size the array for LMC_MAX_RUN_STREAMS): consecutive run() calls chain up per sub-block, and the tail of one
 *        sub-block's launch is covered by the others' next launch. Every other
 *        entry point (and lmc_engine_synchronize) is ordered after all launched sub-blocks; work on the engine's
 *        stream that precedes a run() is ordered before it.
 * run_streams(): the streams run() launches its kernels on (returns their number, at most `capacity` written) -- for
 *        callers that bracket launches with their own timing events. */
/* step_rand (base_hmc.py:46,123,154-155) in the one form that keeps same-seed parity on the device:
 * step_rand = lambda s: s * np.random.uniform(lo, hi) -- one double of the chain's own stream per iteration, drawn
 * between the start state and the trajectory. enable = 0 switches it off (the default). */
int lmc_engine_set_step_jitter(lmc_engine* e, int32_t enable, double lo, double hi);
/* step_rand as an ARBITRARY host function (base_hmc.py:46,123,154-155: `step_size = self._step_rand(step_size)` once per
 * iteration): the caller evaluates it for every chain and hands the results over; the next lmc_engine_run() integrates
 * with step_sizes[chain] (HOST or DEVICE pointer, [chains]) instead of exp(log_step) / exp(log_bar) -- run ONE iteration
 * per call and refresh the values in between. NULL switches back -- to the adapted step sizes, or to the device's own jitter if
 * lmc_engine_set_step_jitter() enabled one (before or while the override was in force). Dual averaging is untouched (the reference adapts the
 * un-jittered step size too). */
int lmc_engine_set_step_sizes(lmc_engine* e, const double* step_sizes);
/* potential.update(sample = the chain's current position, grad, tune) of QuadPotentialDiagAdapt for every chain as a call
 * of its own (quadpotential.py:231-245; the fixed potentials' update is the base class's `pass`, :112-118): the device
 * function lmc_engine_run() applies after every tuning iteration. The dense counterpart is lmc_engine_dense_update(). */
int lmc_engine_diag_update(lmc_engine* e, int32_t tune);
int lmc_engine_reserve(lmc_engine* e, int64_t capacity, int64_t trace_begin);
/* Thinning: reserve() for a job that keeps every thin-th draw. Of the iterations trace_begin, trace_begin + 1, ... the
 * sampling kernels store trace_begin, trace_begin + thin, trace_begin + 2 thin, ...: the trace -- in HBM or attached
 * (lmc_engine_attach_trace) -- has ceil((capacity - trace_begin) / thin) rows per chain (lmc_engine_trace_rows), row r
 * holding iteration trace_begin + r * thin, and the discarded draws are never written anywhere. lmc_engine_reserve() is
 * thin = 1. Nothing else changes: the per-draw statistic records stay [chains][capacity], one per ITERATION (counters,
 * lmc_engine_get_stat_*() and the tuned-step statistics need every one of them; at 64 bytes each they are not what fills
 * memory) -- lmc_engine_copy_window_strided_async() exports the kept ones -- and adaptation, moments and counters see every
 * draw. thin < 1 is LMC_ERR_INVALID. On a thinned engine lmc_engine_get_trace(dst, iter_begin, n_iters) delivers the kept
 * iterations inside [iter_begin, iter_begin + n_iters), in order (dst: [chains][that many][dim]).
 * Limits: with thin > 1 the capacity may be at most 2^29 iterations (LMC_ERR_INVALID beyond: the kernels count kept draws
 * in 32 bits). A thin larger than the capacity keeps iteration trace_begin alone, exactly like thin = capacity, and is
 * applied as such inside the library; lmc_engine_thin() still returns the value as it was given. */
int lmc_engine_reserve_thinned(lmc_engine* e, int64_t capacity, int64_t trace_begin, int64_t thin);
int64_t lmc_engine_thin(lmc_engine* e);          /* as given to reserve_thinned(); 1 after reserve() */
int64_t lmc_engine_trace_rows(lmc_engine* e);    /* rows per chain of the trace; 0: no trace */
/* The arithmetic of thinning, as the library does it for every launch (pure; no engine, no device): of the iterations
 * [first, first + n), those kept under (trace_begin, thin) are *first_kept, *first_kept + thin, ... (*n_kept of them; 0:
 * none, *first_kept is then the next kept iteration at or after first + n), and *first_kept lies in trace row *first_row.
 * Out pointers may be NULL. */
int lmc_thin_window(int64_t first, int64_t n, int64_t trace_begin, int64_t thin, int64_t* first_kept, int64_t* n_kept, int64_t* first_row);
/* Where the draws go, decided after reserve(capacity, trace_begin < 0) and possibly while the job is already running (the
 * kernel arguments of a launch are fixed when it is enqueued: launches enqueued AFTER this call store the draws of iterations
 * >= trace_begin, so call it before enqueueing the first launch that reaches trace_begin).
 *   dst != NULL: the caller's own array [chains][capacity - trace_begin][dim] in device-accessible memory (page-locked host
 *        memory: lmc_host_alloc / lmc_host_register; or device memory). The sampling kernel stores every draw THERE, one
 *        coalesced row per chain per iteration, straight over the host link as it is produced -- the array sample() returns
 *        (sampling.py:207-222) is complete when the last launch is, with no copy and no trace in HBM. The engine never frees
 *        it; lmc_engine_get_trace() / trace_device_ptr() read through it. On a thinned engine (lmc_engine_reserve_thinned) the
 *        array is [chains][ceil((capacity - trace_begin) / thin)][dim].
 *   dst == NULL: the engine allocates the trace in HBM (what reserve(capacity, trace_begin) does). */
int lmc_engine_attach_trace(lmc_engine* e, double* dst, int64_t trace_begin);
/* KeyboardInterrupt (sampling.py:324-328, :470-471: the reference keeps what has been drawn so far). stop = 1: every
 * chain leaves the launch it is in at the end of an iteration within ~16 iterations, and a workgroup that STARTS under the
 * request does nothing at all -- launches still queued neither run an iteration nor touch iter_count, and chains of the
 * current launch whose wavefronts had not started yet stay where the previous launch left them. The stop word is pinned
 * host memory that one chain in at most 256 of a launch (taking turns) polls and copies to a device word, so the request
 * needs nothing scheduled on the device. Chains end at different iterations: lmc_chain_state.iter_count says where; draws
 * and statistics below its MINIMUM are complete for every chain. Consequence for callers: with many more chains than
 * resident wavefront slots (lmc_engine_occupancy), a launch is the granularity at which the not-yet-started chains are
 * cut off -- littlemcmc_amd.sample() therefore cuts such jobs into launches of at most 500 iterations. stop = 0 re-arms
 * the engine, ordered after everything launched so far. Fused, dense and general kernels; a tick-driven job stops by not
 * ticking. */
int lmc_engine_request_stop(lmc_engine* e, int32_t stop);
/* The `callback` of the reference's drivers (sampling.py:272-277, :307-308: called per draw, "sampling can be interrupted
 * by throwing a KeyboardInterrupt in the callback") needs to know where a running job is WITHOUT waiting for it:
 * progress() is the iteration index a relay chain of the launch in flight last started, read from pinned host memory (no
 * stream is touched; updated every 16th iteration). A hint: chains advance at their own pace; what every chain has
 * completed is lmc_chain_state.iter_count. */
int64_t lmc_engine_progress(lmc_engine* e);
int lmc_engine_run(lmc_engine* e, int64_t n_tune, int64_t iter_begin, int32_t n_iters);
#define LMC_MAX_RUN_STREAMS 8
int lmc_engine_run_streams(lmc_engine* e, void** streams, int32_t capacity);
/* The LDS plan (LMC_LDS_PLAN_SHALLOW / _DEEP) of the most recent lmc_engine_run() launch; 0 before the first launch and for
 * engines whose kernels have one plan only. lmc_engine_run_lds_bytes() reports the bytes of that launch. */
int32_t lmc_engine_last_run_plan(lmc_engine* e);
/* The leaf-group width of the NUTS tree build the most recent lmc_engine_run() launch ran (2 = leaf pairs, 4 = leaf quads;
 * lmc_tuning.leaf_group); 0 before the first launch and for kernels that do not build trees in groups. */
int32_t lmc_engine_last_run_leaf_group(lmc_engine* e);
/* The dense kernel the most recent lmc_engine_run() launched: 1 = one chain per wavefront with its own matrix sweep
 * (run_dense_kernel), 2 = eight chains per workgroup around the shared matrix in LDS (run_dense_coop_kernel,
 * LMC_POT_FULL up to model_ndim 128, lmc_tuning.dense_coop_off switches it off); 0 before the first launch and for
 * engines without a dense matrix or on the general kernels. */
int32_t lmc_engine_last_run_dense_kernel(lmc_engine* e);

/* ---- results (synchronise the stream). dst shapes: trace [chains][n_iters][dim]; stats [chains][n_iters] */
int lmc_engine_get_trace(lmc_engine* e, double* dst, int64_t iter_begin, int64_t n_iters);
int lmc_engine_get_stat_f64(lmc_engine* e, int32_t stat, double* dst, int64_t iter_begin, int64_t n_iters);
int lmc_engine_get_stat_i32(lmc_engine* e, int32_t stat, int32_t* dst, int64_t iter_begin, int64_t n_iters);
int lmc_engine_get_stat_u8(lmc_engine* e, int32_t stat, uint8_t* dst, int64_t iter_begin, int64_t n_iters);
/* ---- results, streamed: sampling.py:207-222 hands the caller host arrays; a job's draws are tens of GiB (C3: 64 GiB), so the
 * copy must not wait for the job. copy_window_async() enqueues, on a high-priority copy stream of the engine's own, the device->host
 * copy of iterations [iter_begin, iter_begin + n_iters) of EVERY chain into the caller's final arrays, ordered after every
 * lmc_engine_run() enqueued so far and asynchronous to the host and to later launches (the D2H of launch k runs under
 * launch k + 1). Destinations are laid out like the reference's results -- trace [chains][n_out][dim], planes [chains][n_out] --
 * and iteration `first` lands in row 0; a plane is one statistic out of the per-draw records, converted on the device to the
 * dtype the reference's stats dict carries (nuts.py:87-101, hmc.py:36-50). The copies are kernels that write the
 * destinations themselves (coalesced stores over the host link, no per-row DMA command), so the destinations must be
 * DEVICE-ACCESSIBLE: page-locked host memory (lmc_host_alloc, or memory registered with hipHostRegister) or device
 * memory; pageable memory is refused with LMC_ERR_INVALID. copy_wait() waits for the copies enqueued so far (and
 * nothing else). */
#define LMC_PLANE_F64 0      /* idx = LMC_STAT_* f64 slot */
#define LMC_PLANE_I32 1      /* idx = LMC_STAT_DEPTH / LMC_STAT_TREE_SIZE */
#define LMC_PLANE_U8 2       /* idx = LMC_STAT_DIVERGING / _TUNE / _ACCEPTED */
#define LMC_AS_NATIVE 0      /* float64 / int32 / uint8 as stored */
#define LMC_AS_F64 1         /* written as float64 (the reference's "tree_size" is float64) */
#define LMC_AS_I64 2         /* written as int64 (the reference's "depth", HMC's "n_steps") */
#define LMC_MAX_PLANES 16
typedef struct lmc_window_plane {
    void* dst;               /* [chains][n_out] of the output dtype */
    int32_t kind;            /* LMC_PLANE_* */
    int32_t idx;
    int32_t as;              /* LMC_AS_* */
    int32_t reserved;
} lmc_window_plane;
typedef struct lmc_window_dst {
    int64_t n_out;           /* iterations per chain the destination arrays hold */
    int64_t first;           /* iteration index that lands in destination row 0 */
    double* trace;           /* [chains][n_out][dim], or NULL */
    int32_t n_planes;
    int32_t copy_workgroups; /* single-wavefront workgroups a window copy may use; 0 = the default (64): enough to saturate the
                              * host link, few enough to leave the wave slots to the sampling launches it runs under */
    lmc_window_plane plane[LMC_MAX_PLANES];
} lmc_window_dst;
int lmc_engine_copy_window_async(lmc_engine* e, const lmc_window_dst* dst, int64_t iter_begin, int64_t n_iters);
/* The same for a destination that keeps every stride-th iteration: its n_out ROWS hold the iterations dst->first,
 * dst->first + stride, ...; of the window [iter_begin, iter_begin + n_iters) the iterations with (it - dst->first) % stride
 * == 0 are written, into row (it - dst->first) / stride of every plane (the gather kernel is indexed by destination row:
 * it = first + row * stride). dst->trace != NULL copies the same rows out of the engine's HBM trace, which must hold exactly
 * those iterations: stride == the engine's thin and (dst->first - trace_begin) % stride == 0, else LMC_ERR_INVALID.
 * copy_window_async() is stride = 1. */
int lmc_engine_copy_window_strided_async(lmc_engine* e, const lmc_window_dst* dst, int64_t iter_begin, int64_t n_iters, int64_t stride);
int lmc_engine_copy_wait(lmc_engine* e);
/* Page-locked host memory every visible GPU can copy into (hipHostMalloc, portable): what the arrays sample() returns live
 * in. NULL on failure (lmc_last_error(NULL)); free with lmc_host_free. */
void* lmc_host_alloc(uint64_t bytes);
void lmc_host_free(void* p);
/* Page-lock (and map into every GPU) a range of memory the caller already owns -- e.g. an anonymous mapping it has
 * pre-faulted from several threads: pinning is dominated by the kernel zeroing fresh pages, which one thread does at
 * ~12 GiB/s; disjoint ranges may be registered concurrently from several threads. Unregister before unmapping. */
int lmc_host_register(void* p, uint64_t bytes);
int lmc_host_unregister(void* p);

/* Device pointers of the engine-owned outputs for zero-copy consumers; valid until the next reserve()/destroy().
 * Trace: [chains][lmc_engine_trace_rows()][dim] float64 (capacity - trace_begin rows unless thinned). Statistics: [chains][capacity] records of LMC_STAT_RECORD_BYTES
 * = 64 bytes, one per draw, written by the sampling kernel in one coalesced store:
 *     bytes  0..55  the seven float64 statistics in LMC_STAT_* (f64) order
 *     bytes 56..59  int32  tree_size (NUTS) / n_steps (HMC): the leapfrog steps of the draw
 *     bytes 60..63  uint32 bits 0-15 NUTS depth, bit 16 diverging, bit 17 tune, bit 18 accepted
 * (lmc_engine_get_stat_*() gather one statistic out of the records into a dense [chains][n_iters] array.) */
#define LMC_STAT_RECORD_BYTES 64
void* lmc_engine_trace_device_ptr(lmc_engine* e);
void* lmc_engine_stat_records_device_ptr(lmc_engine* e);
int64_t lmc_engine_trace_begin(lmc_engine* e);
int64_t lmc_engine_capacity(lmc_engine* e);

/* adaptation state: potential._var [chains][dim] (float32), step_adapt fields [chains][4] =
 * {log_step, log_bar, hbar, mu}, step_adapt._count [chains], potential._n_samples [chains].
 * Any pointer may be NULL. */
int lmc_engine_get_adapt_state(lmc_engine* e, float* var, double* dual_avg, int32_t* da_count,
                               int32_t* n_samples);
/* Full adaptation state of every chain, for checkpoint/resume and for per-iteration parity tests
 * (the reference has no such call: its state is the Python step object, base_hmc.py:192-200).
 * Every pointer may be NULL (skipped). Shapes: vectors [chains][dim], scalars [chains].
 * set(): inv_std is re-derived from var exactly as quadpotential.py:226-229 does (float32 sqrt, 1/x). */
typedef struct lmc_chain_state {
    float* var;             /* potential._var */
    double* fore_mean;      /* potential._foreground_var.mean */
    double* fore_raw_var;   /* potential._foreground_var.raw_var */
    double* back_mean;      /* potential._background_var.mean */
    double* back_raw_var;   /* potential._background_var.raw_var */
    double* fore_w_sum;     /* potential._foreground_var.w_sum */
    double* back_w_sum;     /* potential._background_var.w_sum */
    int32_t* n_samples;     /* potential._n_samples */
    double* log_step;       /* step_adapt._log_step */
    double* log_bar;        /* step_adapt._log_bar */
    double* hbar;           /* step_adapt._hbar */
    int32_t* da_count;      /* step_adapt._count */
    int32_t* iter_count;    /* step.iter_count */
    int32_t* window;        /* potential.adaptation_window (grows by the multiplier at every switch) */
    double* var64;          /* potential._var of a float64 QuadPotentialDiagAdapt (general kernels only; LMC_ERR_STATE otherwise) */
} lmc_chain_state;
int lmc_engine_get_chain_state(lmc_engine* e, const lmc_chain_state* dst);
int lmc_engine_set_chain_state(lmc_engine* e, const lmc_chain_state* src);
/* Dense-potential state of every chain (FULL_ADAPT: per chain; FULL / FULL_INV: get() replicates the shared
 * matrices). Matrices [chains][dim][dim] row-major in the reference's orientation, vectors [chains][dim],
 * scalars [chains]; NULL = skipped. set() is for checkpoint / resume and per-iteration parity tests. */
typedef struct lmc_dense_state {
    float* cov;              /* potential._cov (FULL_INV: float32 of A^-1, get only) */
    float* chol;             /* potential._chol, lower (FULL_INV: float32 of L, get only) */
    double* fore_mean;       /* potential._foreground_cov.mean */
    double* fore_raw_cov;    /* potential._foreground_cov.raw_cov */
    double* fore_n;          /* potential._foreground_cov.n_samples */
    double* back_mean;
    double* back_raw_cov;
    double* back_n;
    int32_t* window;         /* potential._adaptation_window */
    int32_t* previous_update;/* potential._previous_update */
    int32_t* chol_failures;  /* refreshes whose factorisation failed: potential._chol_error is not None */
    double* cov64;           /* cov / chol as float64: what QuadPotentialFullAdapt(dtype="float64") (cfg.mass_f64) holds; the */
    double* chol64;          /* float32 potentials' values widened. set(): either form of a matrix, not both */
} lmc_dense_state;
int lmc_engine_get_dense_state(lmc_engine* e, const lmc_dense_state* dst);
int lmc_engine_set_dense_state(lmc_engine* e, const lmc_dense_state* src);
/* cov / chol [dim][dim] of ONE chain (the host mirror of step.potential after sample()). */
int lmc_engine_get_dense_chain(lmc_engine* e, int32_t chain, float* cov, float* chol);
int lmc_engine_get_dense_chain_f64(lmc_engine* e, int32_t chain, double* cov, double* chol);   /* (float64 potentials: unrounded) */
/* The lower Cholesky factor [dim][dim] in float64 of the float64 potentials: QuadPotentialFull(cov, dtype="float64")._chol
 * (quadpotential.py:441-443) / QuadPotentialFullInv.L (:402), as the device holds it. */
int lmc_engine_get_dense_factor_f64(lmc_engine* e, double* chol);
/* Test entry: potential.update(sample = current position, grad, tune) for every chain (quadpotential.py:528-552).
 * During lmc_engine_run() the same kernel runs after every tuning iteration. */
int lmc_engine_dense_update(lmc_engine* e, int32_t tune);

/* ---- one shared dense matrix adapted from ALL chains (LMC_POT_FULL, dim <= 256, fused kernels; other potentials:
 * LMC_ERR_STATE, larger dim: LMC_ERR_INVALID). The reference has no such estimator: its adaptive dense potential learns one
 * matrix per chain from that chain's own draws (quadpotential.py:471-557); with C chains one iteration already holds C draws of
 * the target. The engine keeps, in float64 on the device,
 *     n,  shift[dim],  s = sum (q - shift),  S = sum (q - shift)(q - shift)^T
 * over SNAPSHOTS of the current positions of all chains; shift is the column mean of the first snapshot after a reset, so that
 * S - s s^T / n has no cancellation to speak of. The sums are formed without floating-point atomics in an order that depends
 * on the chain count alone: the same positions give the same bits.
 * pool_reset():      zero the statistic. Asynchronous.
 * pool_accumulate(): one snapshot. Asynchronous: ordered after every lmc_engine_run() enqueued so far, and the next
 *                    lmc_engine_run() is ordered after it; the host does not wait. At least 2 chains.
 * pool_get():        synchronises. n, mean = shift + s / n [dim], m2 = S - s s^T / n [dim][dim] (symmetric). Any pointer may be NULL.
 * pool_apply():      synchronises. cov = m2 / (n - 1), shrunk as Stan does, cov <- n / (n + 5) cov + 1e-3 * 5 / (n + 5) I, then
 *                    installed as the engine's shared matrix exactly as lmc_engine_set_dense_potential(cov) installs one.
 *                    n < 2, a non-finite entry or a failed factorisation: LMC_ERR_INVALID, the installed matrix stays.
 * restart_dual_average(): per chain mu <- log(10 exp(log_step)), hbar <- 0, log_bar <- 0, count <- 1 (log_step stays): Stan's
 *                    restart of step-size adaptation after a change of metric. Asynchronous. */
int lmc_engine_pool_reset(lmc_engine* e);
int lmc_engine_pool_accumulate(lmc_engine* e);
int lmc_engine_pool_get(lmc_engine* e, int64_t* n, double* mean, double* m2);
int lmc_engine_pool_apply(lmc_engine* e);
int lmc_engine_restart_dual_average(lmc_engine* e);

/* ---- externally evaluated density (cfg.target_family = LMC_TARGET_EXTERNAL): the iteration loop of
 * sampling.py:507-521 / base_hmc.py:140-190 cut at the two places the reference calls logp_dlogp_func
 * (integration.py:62 compute_state, :115 _step). Protocol:
 *     lmc_engine_reserve(); lmc_engine_tick_begin(n_tune, iter_begin, n_iters);
 *     do { evaluate (logp[chains], grad[chains][dim]) at lmc_engine_tick_positions() [chains][dim];
 *          lmc_engine_tick(logp, grad, &n_active); } while (n_active > 0);
 * All three arrays are DEVICE memory. Every tick advances every unfinished chain by exactly one density
 * evaluation, whatever iteration or tree depth it is in; finished chains ignore their inputs. Passing
 * n_active = NULL skips the host synchronisation (poll every few ticks instead). */
int lmc_engine_tick_begin(lmc_engine* e, int64_t n_tune, int64_t iter_begin, int32_t n_iters);
void* lmc_engine_tick_positions(lmc_engine* e);
int lmc_engine_tick(lmc_engine* e, const double* logp, const double* grad, int32_t* n_active);

/* Running per-chain moments of the post-warm-up draws, kept on the device so that cross-chain R-hat needs no
 * trace (the only quantities the multi-GPU gather moves): mean [chains][dim], m2 = sum of squared
 * deviations [chains][dim], n [chains]. Enable before reset_tuning(); reset with it. */
int lmc_engine_keep_moments(lmc_engine* e, int32_t enable);
int lmc_engine_get_moments(lmc_engine* e, double* mean, double* m2, int32_t* n);
int lmc_engine_get_status(lmc_engine* e, int32_t* status);
int lmc_engine_get_counters(lmc_engine* e, int64_t* counters);

/* ---- unit entry points --------------------------------------------------------------------------
 * trajectory(): integrator.compute_state(q0, p0) followed by n_fwd steps of +eps and n_back steps of
 * -eps (integration.py:52-121), every chain from its own (q0, p0) [chains][dim]. Outputs hold
 * n_fwd + n_back + 1 states: q/p/v/g [chains][n_states][dim], energy/logp [chains][n_states].
 * p0_is_f32 selects the float32 start-state dtype flow of QuadPotentialDiagAdapt. */
int lmc_engine_trajectory(lmc_engine* e, const double* q0, const double* p0, int32_t p0_is_f32,
                          double eps, int32_t n_fwd, int32_t n_back, double* out_q, double* out_p,
                          double* out_v, double* out_g, double* out_energy, double* out_logp);
/* logp_dlogp_func(q) for every chain: q [chains][dim] -> logp [chains], grad [chains][dim]. */
int lmc_engine_logp_dlogp(lmc_engine* e, const double* q, double* logp, double* grad);
/* Draw from every chain's stream: ops[i] > 0 -> normal(size=ops[i]); ops[i] < 0 -> -ops[i] uniforms.
 * out [chains][sum |ops|]. */
int lmc_engine_rng_draw(lmc_engine* e, const int32_t* ops, int32_t n_ops, double* out);
/* potential.random() for every chain (quadpotential.py:221-224 / :374-376): out [chains][dim]. */
int lmc_engine_draw_momentum(lmc_engine* e, double* out);
/* What the counter-based streams hand iteration `iteration` of every chain (a pure function of lmc_engine_seed's seeds):
 * normals  [chains][dim]: the standard normals of the momentum draw, before the mass scaling (NULL: not wanted)
 * uniforms [chains][n_uniforms]: the first n_uniforms decision uniforms in consumption order (NULL: not wanted)
 * LMC_ERR_INVALID on the numpy stream. */
int lmc_engine_counter_draws(lmc_engine* e, int64_t iteration, double* normals, double* uniforms, int32_t n_uniforms);

/* ---- a user-written density compiled at run time (cfg.target_family = LMC_TARGET_USER in the stock library) ------------
 * The kernels that depend on the density functor -- run_kernel<run_ns, run_w, UserTarget>, trajectory_kernel<unit_ns,
 * UserTarget>, logp_kernel<unit_ns, UserTarget> (csrc/lmc_sampler.hpp, csrc/lmc_unit_kernels.hpp) -- are compiled by the
 * caller with hiprtc for the shape lmc_engine_kernel_shape() reports, and handed over as a code object plus the three
 * (lowered) kernel names; everything else stays the prebuilt library. This is how `logp_dlogp_func` (integration.py:
 * 40,62,115) becomes a device function linked into the leapfrog kernel without hipcc on the machine. Diagonal mass
 * matrices only; littlemcmc_amd.targets.UserTarget drives it. */
int lmc_engine_kernel_shape(lmc_engine* e, int32_t* unit_ns, int32_t* run_ns, int32_t* run_w);
/* 1 if this engine runs the general kernels ("Which kernels an engine runs", above): one wavefront per chain up to dim 512
 * (run_w = 1), sixteen beyond (run_w = 16); a run-time compiled density then instantiates run_wide_kernel<run_ns, run_w,
 * UserTarget>, wide_trajectory_kernel and wide_logp_kernel instead of the fused kernels. */
int32_t lmc_engine_uses_general_kernels(lmc_engine* e);
/* How the sampling kernel of this engine occupies the GPU (asked of the HIP runtime for the very kernel, block size and
 * dynamic LDS lmc_engine_run() launches with): resident_chains = chains that run concurrently (compute units x
 * workgroups per unit; 0 for engines without a fused sampling kernel), waves_per_chain, and the rate of the constant
 * wall clock LMC_CT_WAVE_TICKS counts in. The host uses it to size launches (the reference's analogue is `cores`,
 * sampling.py:117-129). Any pointer may be NULL. */
int lmc_engine_occupancy(lmc_engine* e, int32_t* resident_chains, int32_t* waves_per_chain, double* wall_clock_hz);
/* Dynamic LDS bytes per workgroup (= per chain) of the sampling kernel lmc_engine_run() launches; rocprofv3's kernel trace
 * lists only the static part (0). Negative: no fused diagonal-mass kernel. */
int32_t lmc_engine_run_lds_bytes(lmc_engine* e);
int lmc_engine_load_user_kernels(lmc_engine* e, const void* code_object, const char* run_name, const char* trajectory_name,
                                 const char* logp_name);
/* Optional, after lmc_engine_load_user_kernels(): the name of run_kernel<NS, 1, UserTarget, 0, 1> in the same code object -- the
 * one-wave sampling kernel under the deep-tree LDS plan (stack level 2 in LDS, MT19937 used in place; csrc/lmc_sampler.hpp).
 * With it the engine chooses the plan of every launch from the tree sizes the running chains report, as it does for the
 * built-in densities (results do not depend on the choice); without it a run-time compiled density runs under plan 0. */
int lmc_engine_load_user_run_plan1(lmc_engine* e, const char* run_name_plan1);

/* ---- cross-chain diagnostics on the draws in HBM (the reference has none: ArviZ recipe only,
 * docs/tutorials/framework_cookbook.rst:201-213) -------------------------------------------------------------------
 * Per-dimension sufficient statistics of the sub-series [t0, t0 + n) of every chain of a trace block
 * x[chains][draws_stride][dim] (DEVICE pointer, e.g. lmc_engine_trace_device_ptr()):
 *   out[0][dim] = sum over chains of the chain mean          out[1][dim] = sum of squared chain means
 *   out[2][dim] = sum of unbiased within-chain variances (lag0 == 0 only, else 0)
 *   out[3 + k][dim] = sum of biased (1/n) autocovariances at lag lag0 + k, k < lmc_diag_lags_per_pass()
 * out is a DEVICE pointer to (3 + lags_per_pass) * dim doubles. The work is enqueued on `stream` (a hipStream_t, NULL =
 * default stream) of the current device; the result is bit-reproducible (no floating-point atomics). The statistics add
 * over chains, chain halves and ranks: split R-hat and the Geyer ESS follow from their sums (littlemcmc_amd/diagnostics.py).
 * Refused with LMC_ERR_INVALID before any HIP call: NULL x or out, chains outside [1, 2^31) (chain indices are 32-bit in the
 * group arithmetic this call shares with the grouped one below), dim < 1, n < 2, t0 < 0, t0 + n > draws_stride, lag0 < 0. */
int lmc_diag_lags_per_pass(void);
int lmc_diag_chain_stats(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                         int32_t lag0, double* out, void* stream);
/* Additive within ABI 9: the same statistics PER GROUP of chains (many posteriors in one job, targets.Batched) in one pass.
 * x is a trace block whose chain 0 is chain first_chain of the job; chain c of the block belongs to group
 * (first_chain + c) / chains_per_group (lmc_target_param_row). The block touches the groups g0 = first_chain / chains_per_group
 * .. g1 = (first_chain + chains - 1) / chains_per_group, and out is [g1 - g0 + 1][3 + lags_per_pass][dim] doubles (DEVICE):
 * the block above once per touched group, in group order. A first or last group that lies only partly inside the block
 * gets the sums over its chains that are present -- the statistics add over chains, so the parts of a group that straddles
 * two blocks (two GPUs) are simply added. Bit-reproducible like the ungrouped call, which IS this call with first_chain 0
 * and chains_per_group = chains. Refused with LMC_ERR_INVALID before any HIP call: what lmc_diag_chain_stats refuses,
 * first_chain < 0, chains_per_group < 1, first_chain + chains outside [1, 2^31). */
int lmc_diag_chain_stats_grouped(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                 int32_t lag0, int64_t first_chain, int64_t chains_per_group, double* out, void* stream);

/* ---- pointwise predictive pass over the draws in HBM, GLM family (additive within ABI 9; littlemcmc_amd/predictive.py:
 * lppd, WAIC, held-out scoring) ------------------------------------------------------------------------------------------
 * x, chains, draws_stride, dim, t0, n: the trace block and sub-series of lmc_diag_chain_stats (a draw is dim contiguous
 * doubles, chains lie draws_stride rows apart). rows is a DEVICE table [n_rows][row_len] of parameter rows in the
 * LMC_TARGET_GLM layout -- the rows the chains were sampled with, or rows of held-out data of the same dim; chain c of the
 * block belongs to group (first_chain + c) / chains_per_group (lmc_target_param_row) and is scored on that group's row. With
 * l[s, i] the pointwise log-likelihood of draw s at observation i -- the l_n of LMC_TARGET_GLM above, constants dropped -- and
 * the block touching groups g0 .. g1, out is [g1 - g0 + 1][6][npad] doubles (DEVICE), npad that of the rows; per group and
 * observation, over the n_g draws of the group that lie in x, rows [t0, t0 + n):
 *   [0] n_g (as a double)   [1] m = max_s l   [2] S = sum_s exp(l - m)   [3] mean_s l   [4] M2 = sum_s (l - mean)^2
 *   [5] sum_s mu, mu the mean response: sigmoid(eta) (bernoulli), exp(eta) (poisson), eta (gaussian)
 * so that log mean_s exp(l) = m + log S - log n_g. Two blocks a, b of draws merge by m = max(ma, mb),
 * S = Sa exp(ma - m) + Sb exp(mb - m), Chan's update mean = mean_a + (mean_b - mean_a) nb / n,
 * M2 = M2a + M2b + (mean_b - mean_a)^2 na nb / n, sums for [0] and [5]; a block of count 0 is skipped by its count. A group
 * that lies only partly in x gets the block of its draws that are present; the parts merge by the same rule (two GPUs).
 * Observations i >= N (padding up to npad) hold finite values of no meaning. Bit-reproducible: no floating-point atomics,
 * chain blocks merged in a fixed order.
 * Non-finite l: a draw with l = -inf (the poisson exp(eta) overflowed) counts in [0] and contributes exp(l - m) := 0 to S
 * whatever m is, so [1] and [2] are those of the other draws and m + log S stays finite (every draw -inf: m = -inf, S = 0);
 * [3] and [4] are then non-finite (-inf or NaN) and [5] is +inf. A NaN l makes [1] .. [5] of that observation NaN.
 * Refused with LMC_ERR_INVALID before any HIP call: NULL x, rows or out; what lmc_diag_chain_stats_grouped refuses for
 * chains, dim, t0, first_chain and chains_per_group; n < 1 or t0 + n > draws_stride (one draw is a block like any other:
 * nothing here divides by n - 1); dim > LMC_GLM_MAX_DIM; a row_len that no N gives at that dim; a touched group >= n_rows.
 * Then the headers of the touched rows are read back in one copy on `stream` (the call's one host look, before any launch),
 * and a header that disagrees with dim or row_len or carries an unknown likelihood code is refused the same way. */
int lmc_glm_pointwise(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                      const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                      double* out, void* stream);

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out on the draws in HBM (additive within ABI 9; Vehtari,
 * Gelman, Gabry 2017; littlemcmc_amd/predictive.py: psis, loo) --------------------------------------------------------------
 * lmc_glm_pointwise_loglik WRITES the pointwise log-likelihood that lmc_glm_pointwise only reduces. x .. chains_per_group are
 * the arguments of lmc_glm_pointwise, with one more demand: the trace block holds WHOLE groups, first_chain % chains_per_group
 * == 0 and chains % chains_per_group == 0 (a row of the result is all the draws of one posterior). With G = chains /
 * chains_per_group groups in the block, the observation blocks [ob0, ob1) (64 observations a block, 0 <= ob0 < ob1 <=
 * npad / 64) and S = chains_per_group * n, out is [G][(ob1 - ob0) * 64][S] doubles (DEVICE):
 *   out[group][(ob - ob0) * 64 + lane][s] = l[s, 64 ob + lane],   s = (chain within the group) * n + t,  t in [0, n)
 * so every (group, observation) row is S contiguous doubles, chains n apart. l is THE SAME BITS lmc_glm_pointwise reduces
 * (one device function computes it for both kernels): max_s of a row equals plane [1] of lmc_glm_pointwise exactly. Padding
 * observations (i >= N) hold finite values of no meaning.
 * Refused with LMC_ERR_INVALID before any HIP call: what lmc_glm_pointwise refuses before its header copy; a block that does
 * not hold whole groups; ob0 < 0, ob1 <= ob0, ob1 > npad / 64; chains * (ob1 - ob0) >= 2^31. Then the same header check. */
int lmc_glm_pointwise_loglik(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                             const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                             int64_t ob0, int64_t ob1, double* out, void* stream);

/* PSIS of `rows` independent rows of S log-likelihood values: row r is l[r * row_stride .. + S) (DEVICE, row_stride >= S);
 * nothing beyond a row's S values is read. The call knows nothing of GLMs. out is [rows][8] doubles (DEVICE):
 *   [0] elpd   [1] pareto_k   [2] n_tail   [3] sigma (the GPD scale)   [4] ess_w = (sum w)^2 / sum w^2 of the final weights
 *   [5] the cutoff (a shifted log ratio)   [6] min_s l   [7] 0
 * One row, with M = tail_len (the host passes min(S / 5, ceil(3 sqrt(S / reff))); for S = 1, M = 0):
 *  1. lw_s = -l_s - c, c = max_s(-l_s), so max lw = 0. If any l_s is NaN or +-inf: [0], [1], [3], [4], [5] are NaN, [2] = 0
 *     and [6] is NaN (some NaN) or the plain min; no other row is affected.
 *  2. cutoff = the (M + 1)-th largest lw, but at least log(DBL_MIN) = -708.3964185322641. The tail is {s : lw_s > cutoff},
 *     n_tail its size: at most M, fewer when values tie with the cutoff.
 *  3. n_tail <= 4: k = +inf, sigma = NaN, no smoothing. Otherwise the tail is sorted by ascending lw (equal lw: by descending
 *     l), x_i = exp(lw_(i)) - exp(cutoff), i = 1 .. n_tail, and the generalised Pareto fit of Zhang and Stephens (2009) with
 *     the weakly informative priors of Vehtari et al. is: m = 30 + floor(sqrt(n_tail));
 *     b_j = (1 - sqrt(m / (j - 0.5))) / (3 x_(floor(n_tail / 4 + 0.5))) + 1 / x_(n_tail), j = 1 .. m (1-based order statistics);
 *     k_j = mean_i log1p(-b_j x_i);  L_j = n_tail (log(-b_j / k_j) - k_j - 1);  w_j = 1 / sum_l exp(L_l - L_j);
 *     b = sum_j b_j w_j;  k = mean_i log1p(-b x_i);  sigma = -k / b;  finally k <- (n_tail k + 5) / (n_tail + 10).
 *  4. If k is finite, the i-th smallest tail element's lw becomes log(exp(cutoff) + sigma expm1(-k log1p(-p_i)) / k),
 *     p_i = (i - 0.5) / n_tail; then every tail lw above 0 is set to 0.
 *  5. elpd = log sum_s exp(lw_s + l_s) - log sum_s exp(lw_s), evaluated as -c + log A - log B with
 *     A = (S - n_tail) + sum_tail exp(lw'_i - lw_i)  (lw + l = -c for every draw outside the tail, lw' the smoothed value),
 *     B = sum_s w_s, w_s = exp(lw_s) the final weights; ess_w = B^2 / sum_s w_s^2. A constant row gives elpd = l exactly.
 * The cutoff, the tail's membership, n_tail and the order are exact; the sums are taken in a fixed order, so two calls on
 * the same data give the same bits (no floating-point atomics). One workgroup per row; the sorted tail lives in LDS, hence
 * LMC_PSIS_MAX_TAIL. Refused with LMC_ERR_INVALID before any HIP call: NULL l or out; rows outside [1, 2^31); S < 1;
 * row_stride < S; tail_len < 0; tail_len > LMC_PSIS_MAX_TAIL; tail_len >= S when S > 1. */
#define LMC_PSIS_MAX_TAIL 4096
int lmc_psis_rows(const double* l, int64_t rows, int64_t S, int64_t row_stride, int32_t tail_len, double* out, void* stream);

/* ---- exact order statistics of the draws in HBM: one pass of a radix select (additive within ABI 9;
 * littlemcmc_amd/diagnostics.py: order_statistics, quantiles, intervals, tail_ess) ------------------------------------------
 * The order is the IEEE total order on the bits: for u = the 64 bits of a draw v, its key is
 *   K(v) = ~u if the sign bit of u is set, else u | 1 << 63      (unsigned compare of keys:
 *   -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN; u = K & ~(1 << 63) if bit 63 of K is set, else ~K, gives v back).
 * x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group: the trace block, sub-series and groups of
 * lmc_diag_chain_stats_grouped -- the block touches groups g0 .. g1, and a first or last group that lies only partly inside
 * the block is counted over its chains that are present. shift is one of 56, 48, .., 0; prefix is [g1 - g0 + 1][n_ranks][dim]
 * keys (DEVICE) and counts is [g1 - g0 + 1][n_ranks][256][dim] (DEVICE, overwritten):
 *   counts[g][r][b][j] = the number of draws v of dimension j, rows [t0, t0 + n), chains of group g0 + g present in the block,
 *                        with (K(v) >> shift) & 255 == b and, for shift < 56, K(v) >> (shift + 8) == prefix[g][r][j] >> (shift + 8).
 * At shift 56 the prefix is not read (it may be NULL) and n_ranks must be 1. The counts are integers and add over chains,
 * blocks and GPUs exactly: eight passes, after each of which the caller picks per (g, r, j) the bucket where the cumulative
 * count passes the remaining rank, puts its digit into the prefix and subtracts the count below it, leave the key of the
 * wanted order statistic. The work is enqueued on `stream` of the current device (a memset of counts, then one kernel);
 * integer atomics only, so the result does not depend on the order of arrival.
 * Refused with LMC_ERR_INVALID before any HIP call: NULL x or counts; chains, dim or n < 1; t0 < 0 or t0 + n > draws_stride;
 * first_chain < 0, chains_per_group < 1; chains, first_chain + chains or n at or beyond 2^31 (a workgroup's 32-bit counters
 * hold the draws of at least two chains), a result of 2^39 counters or more; a shift that is not a multiple of 8 in 0 .. 56;
 * n_ranks outside 1 .. LMC_SELECT_MAX_RANKS, or not 1 at shift 56; a NULL prefix below shift 56. */
#define LMC_SELECT_MAX_RANKS 16
int lmc_select_digit_counts(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                            int64_t first_chain, int64_t chains_per_group, int32_t shift, int32_t n_ranks,
                            const uint64_t* prefix, int64_t* counts, void* stream);

/* ---- posterior predictions at new X, GLM family (additive within ABI 9; littlemcmc_amd/predictive.py: linear_predictor,
 * predict) ----------------------------------------------------------------------------------------------------------------
 * x .. chains_per_group are the arguments of lmc_glm_pointwise. rows are GLM parameter rows of the POINTS TO PREDICT AT (the
 * LMC_TARGET_GLM layout at the posterior's dim: the training design, or a design whose response is unknown); their y section
 * is NOT READ. [ob0, ob1) are blocks of 64 observations as in lmc_glm_pointwise_loglik; W = (ob1 - ob0) * 64. With
 * eta[s, i] = sum_e X[i][e] q_s[e] the linear predictor of draw s at observation i -- e ascending, one fma per term: the eta of
 * the sampler and of lmc_glm_pointwise, bit for bit (one device function) -- the call has two outputs, either of which may be
 * NULL, not both:
 *   eta    [chains][n][W] doubles (DEVICE): eta[c][t][64 (ob - ob0) + lane] is the linear predictor of draw t0 + t of chain c
 *          of the block at observation 64 ob + lane. This is the [chains, draws, dim] layout of a trace with dim = W and
 *          draws_stride = n, which lmc_select_digit_counts and lmc_diag_chain_stats_grouped read: the exact order statistics
 *          of the predictor are those calls on this array, with the same first_chain and chains_per_group. Whole groups are
 *          not demanded (a chain's rows are its own).
 *   stats  [g1 - g0 + 1][5][W] doubles (DEVICE), the block touching groups g0 .. g1: per group and observation, over the n_g
 *          draws of the group that lie in x, rows [t0, t0 + n):
 *            [0] n_g (as a double)   [1] mean_s eta   [2] M2 = sum_s (eta - mean)^2   [3] mean_s mu   [4] sum_s (mu - mean mu)^2
 *          mu the mean response: sigmoid(eta) (bernoulli), exp(eta) (poisson), eta (gaussian). Two blocks a, b of draws merge
 *          by Chan's update, mean = mean_a + (mean_b - mean_a) nb / n, M2 = M2a + M2b + (mean_b - mean_a)^2 na nb / n, a block
 *          of count 0 skipped by its count; a group that lies only partly in x gets the block of its draws that are present.
 * Observations i >= N (padding up to npad) hold eta = 0. Bit-reproducible: no floating-point atomics; the statistics are
 * two-pass per tile of 8 draws, merged per chain in draw order and then per group in (chain, 256-draw segment) order, a plan
 * that depends on the shape alone -- so two calls, a call on a sub-range of observation blocks and a call without the other
 * output all give the same bits. A non-finite eta or mu (a NaN or infinite coefficient, an overflowing poisson exp(eta))
 * makes the planes [1] .. [4] it enters of THAT (group, observation) non-finite (+-inf or NaN) and touches nothing else; the
 * mu of a NaN eta is NaN, so a NaN coefficient makes all four planes of its group NaN at every observation.
 * Refused with LMC_ERR_INVALID before any HIP call: what lmc_glm_pointwise refuses before its header copy (its `out` aside);
 * ob0 < 0, ob1 <= ob0, ob1 > npad / 64; eta and stats both NULL; chains * n * W >= 2^40 elements of eta (the kernels index
 * with 64 bits; the launch is the limit:) chains * ceil(n / 256) * (ob1 - ob0) >= 2^31. Then the header check of
 * lmc_glm_pointwise, on the touched rows. */
int lmc_glm_linpred(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                    const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                    int64_t ob0, int64_t ob1, double* eta, double* stats, void* stream);

/* ---- posterior co-moments per posterior from the draws in HBM (additive within ABI 9; littlemcmc_amd/diagnostics.py:
 * cross_moments, covariance, contrasts) -------------------------------------------------------------------------------------
 * x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group: the trace block, sub-series and groups of
 * lmc_diag_chain_stats_grouped -- the block touches groups g0 .. g1. For each touched group, over the n_g rows of that group
 * that lie in the block (its chains that are present x the draws [t0, t0 + n)), the call writes (DEVICE, overwritten)
 *   n_out    [g1 - g0 + 1]            n_g as a double
 *   mean_out [g1 - g0 + 1][dim]       the mean row
 *   m2_out   [g1 - g0 + 1][dim][dim]  sum_rows (x - mean)(x - mean)^T, row-major, full and exactly symmetric (the lower
 *                                     triangle is computed and mirrored)
 * Arithmetic (csrc/lmc_cross.hip): shift = the column mean of the group's present rows (per-workgroup column sums, added in
 * workgroup order); s = sum (x - shift) and S = sum (x - shift)(x - shift)^T on v_mfma_f64_16x16x4_f64, per-workgroup
 * partials added in workgroup order; mean = shift + s / n_g, m2 = S - s s^T / n_g. No floating-point atomics, and the split
 * of the rows over workgroups is a function of the shapes alone: the same draws give the same bits. n = 1 is allowed (m2 is
 * all zeros, mean the draw). Two blocks a, b merge by Chan's rule for matrices, m2 = m2a + m2b + (mb - ma)(mb - ma)^T na nb /
 * n, a block of count 0 skipped by its count (diagnostics.merge_cross_moments).
 * A NaN or +-inf in coordinate j of some draw makes mean[j] and row and column j of m2 non-finite; every other entry keeps
 * the bits it has without it (column i's shift reads column i only, and every tile entry is its own dot product).
 * Refused with LMC_ERR_INVALID before any HIP call: what lmc_diag_chain_stats_grouped refuses of the trace view and the
 * grouping (its n >= 2 aside); NULL n_out, mean_out or m2_out; dim > LMC_CROSS_MAX_DIM. */
#define LMC_CROSS_MAX_DIM 512
int lmc_diag_cross_moments(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                           int64_t first_chain, int64_t chains_per_group, double* n_out, double* mean_out, double* m2_out,
                           void* stream);

/* ---- replicated responses y_rep ~ p(y | q_s), GLM family (additive within ABI 9; littlemcmc_amd/predictive.py: replicate,
 * predict_response, ppc; csrc/lmc_yrep.hpp, csrc/lmc_yrep.hip) ---------------------------------------------------------------
 * THE STREAM. The replicated response of draw row r = t0 + t of job chain first_chain + c at observation i of the chain's row
 * is a pure function of (seed, job chain, r, i) and of the draw's eta and mu at i (those of lmc_glm_linpred, bit for bit):
 *   w(b) = philox4x32_10(c0 = r, c1 = i, c2 = b, c3 = 0x6c6d6379 "lmcy", k0 = seed, k1 = job chain),  b = 0, 1, ...
 *   m_j  = (a >> 5) 2^26 + (b >> 6) with (a, b) = words (0, 1) of w(j >> 1) for even j, words (2, 3) for odd j
 *   u_j  = m_j / 2^53 in [0, 1): the 53-bit form of the decision stream (LMC_RNG_COUNTER above)
 * c3 keeps the counter space disjoint from "lmcm" and "lmcu". Nothing lives in memory: a value does not depend on the launch
 * shape, the chunking, the observation-block range, the chain-block partition or the device.
 *   bernoulli  y = (u_0 < mu) ? 1 : 0
 *   gaussian   y = fma(sigma, z, eta), sigma = 1 / sqrt(isig2), z = Phi^-1((m_0 + 1/2) 2^-53) by Wichura's AS 241 (PPND16) in
 *              float64: q = (m_0 - 2^52 + 1/2) 2^-53 exactly; |q| <= 0.425: the central rational in 0.180625 - q^2; otherwise
 *              r = sqrt(-log(min(p, 1 - p))) with the minimum formed exactly as (m_0 + 1/2) 2^-53 or (2^53 - m_0 - 1/2) 2^-53,
 *              and the rational in r - 1.6 (r <= 5) or r - 5, negated for q < 0. No word pair gives p = 0 or 1; z is finite and
 *              antisymmetric in m_0 <-> 2^53 - 1 - m_0. No rejection, no float32.
 *   poisson    lam = mu = exp(eta).  lam = 0: y = 0.  lam < 10, the multiplication method: prod = 1; prod *= u_j for j = 0, 1,
 *              .. until prod <= exp(-lam); y = that j.  lam >= 10, PTRS (Hoermann 1993) as numpy's legacy generator states it:
 *                slam = sqrt(lam), loglam = log(lam), b = 0.931 + 2.53 slam, a = -0.059 + 0.02483 b,
 *                invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2);
 *                attempt t: U = u_(2t) - 0.5, V = u_(2t+1), us = 0.5 - |U|, k = floor((2 a / us + b) U + lam + 0.43);
 *                accept k if us >= 0.07 and V <= vr; reject if k < 0 or (us < 0.013 and V > us); otherwise accept iff
 *                log V + log invalpha - log(a / us^2 + b) <= -lam + k loglam - lgamma(k + 1).
 * eta NaN, mu NaN or mu = +inf give y = NaN, and so does a poisson mu > 2^52. Loops are bounded: after 64 PTRS attempts or 1024
 * uniforms of the multiplication method y = NaN (probability below 1e-30). A count is returned as a double.
 *
 * lmc_glm_yrep: the arguments of lmc_glm_linpred (rows: the points to predict at, their y section NOT READ) and `seed`;
 *   y  [chains][n][W] doubles (DEVICE), W = 64 (ob1 - ob0): y[c][t][64 (ob - ob0) + lane] is the replicated response of draw
 *      t0 + t of chain c at observation 64 ob + lane -- the layout of lmc_glm_linpred's eta, a trace with dim = W, so its
 *      order statistics are lmc_select_digit_counts on it. Observations i >= N (padding) hold 0.
 * Refused with LMC_ERR_INVALID before any HIP call: what lmc_glm_linpred refuses, with `y` NULL in place of both outputs NULL.
 *
 * lmc_glm_yrep_stats: test statistics of every draw's replicated data set, which is never written. rows are the rows of the
 * DATA (all N observations are read, y section included); centre[n_rows] (DEVICE) holds one number per row (the host passes
 * the mean of the row's y). With y_rep_i the value lmc_glm_yrep writes on the same seed, bit for bit (one device function),
 *   T  [chains][n][LMC_YREP_STATS] doubles (DEVICE), per draw over the N real observations of the chain's row g:
 *        [0] sum_i y_rep_i   [1] sum_i (y_rep_i - centre[g])^2   [2] min_i y_rep_i   [3] max_i y_rep_i
 *        [4] the number of y_rep_i == 0
 *        [5] sum_i (y_rep_i - mu_i)^2 / V_i   [6] sum_i (y_i - mu_i)^2 / V_i,  V = mu (1 - mu) | mu | 1 / isig2
 *      a trace-shaped block (dim = 7): lmc_select_digit_counts and the diagnostics read it as they read a trace.
 * Arithmetic is plain (one rounding an operation). A lane accumulates its observations 64 ob + lane over ob ascending; one
 * reduction over the 64 lanes per plane follows -- the balanced tree of the library's wave sum (row_shr 1, 2, 4, 8, row_bcast
 * 15, 31), for [2] and [3] the same tree with a min / max that KEEPS a NaN. A NaN y_rep or V = 0 makes the planes it enters of
 * that draw non-finite and touches no other draw. Bit-reproducible; the mu of a NaN eta is NaN.
 * Refused with LMC_ERR_INVALID before any HIP call: what lmc_glm_pointwise refuses before its header copy (its `out` aside);
 * centre or T NULL; chains * n * 7 >= 2^40. Then the header check of lmc_glm_pointwise, on the touched rows. */
#define LMC_YREP_STATS 7
int lmc_glm_yrep(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                 const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                 int64_t ob0, int64_t ob1, uint32_t seed, double* y, void* stream);
int lmc_glm_yrep_stats(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                       const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                       uint32_t seed, const double* centre, double* T, void* stream);

/* ---- threshold counts of the draws in HBM: which rank a value has (additive within ABI 9; littlemcmc_amd/diagnostics.py:
 * threshold_counts, prob, direction, rope; predictive.exceedance; sbc.sbc_glm; csrc/lmc_threshold.hip) ----------------------
 * x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group: the trace block, sub-series and groups of
 * lmc_select_digit_counts -- the block touches groups g0 .. g1, and a first or last group that lies only partly inside the
 * block is counted over its chains that are present. thresholds is [g1 - g0 + 1][n_thresholds][dim] doubles (DEVICE) and
 * counts is [g1 - g0 + 1][2 n_thresholds + 1][dim] (DEVICE, overwritten). With K = n_thresholds, c = thresholds[g][k][j] and
 * the draws v of dimension j, rows [t0, t0 + n), chains of group g0 + g present in the block:
 *   counts[g][2 k][j]     = the number of draws with v < c
 *   counts[g][2 k + 1][j] = the number of draws with v == c
 *   counts[g][2 K][j]     = the number of draws with v != v (NaN)
 * The comparisons are IEEE NUMERIC comparisons, not the select's total order on the bits: -0.0 == +0.0; a NaN draw is neither
 * below nor equal to anything; a NaN threshold counts 0 and 0; +-inf thresholds and draws compare as numbers. The number of
 * draws above c is the group's draws minus below, equal and NaN. The counts are integers and add over chains, blocks and
 * GPUs exactly. The trace is read once whatever K is. The work is enqueued on `stream` of the current device (a memset of
 * counts, then one kernel); integer atomics only, so the result does not depend on the order of arrival.
 * Refused with LMC_ERR_INVALID before any HIP call: NULL x, thresholds or counts; n_thresholds outside 1 ..
 * LMC_THRESHOLD_MAX; n at or beyond 2^31 (a workgroup's 32-bit counters hold the draws of at least two chains); what
 * lmc_select_digit_counts refuses of the trace view and the grouping; a result of 2^39 counters or more. */
#define LMC_THRESHOLD_MAX 16
int lmc_diag_threshold_counts(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                              int64_t first_chain, int64_t chains_per_group, int32_t n_thresholds, const double* thresholds,
                              int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMC_HIP_H_ */
