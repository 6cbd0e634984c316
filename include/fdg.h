/*
 * fdg.h -- C ABI of the MI355X-native evaluator back end for
 * FeynmanDiagram.jl's static computational graphs.
 *
 * This is the drop-in boundary.  The reference has no
 * FFI for this path; each entry point below names the reference interface it
 * stands in for (paths relative to the reference checkout):
 *
 *   fdg_graph_create      <- Compilers.compile / to_julia_str
 *                            (src/backend/static.jl:98-133, 221-227): the host
 *                            (Julia shim or the Python mirror) walks the graphs
 *                            in the reference's order and hands over the flat
 *                            node table; this call plays the role of
 *                            Meta.parse + @RuntimeGeneratedFunction.
 *   fdg_graph_specialize  <- the JIT step of compile (static.jl:225-226): emits
 *                            a straight-line CDNA4 kernel for this one graph.
 *   fdg_eval              <- the generated eval_graph!(root, leafVal)
 *                            (static.jl:100,131) for B samples at once, in the
 *                            batched layout of compile_Python
 *                            (src/backend/compiler_python.jl:23,28,45-47).
 *   fdg_eval_device       <- same, buffers already resident in HBM.
 *   fdg_accumulate_device <- the user integrand's "sum weight*root over
 *                            samples" step around eval_graph!
 *                            (example/benchmark.jl:58-87), fused so roots never
 *                            travel to HBM.
 *   fdg_fill_uniform_device <- test/bench harness: counter-based leaf values on
 *                            device (the examples draw them from MCIntegration).
 *   fdg_graph_kernel_info <- no counterpart (the reference's evaluator is one Julia function): which hand-written
 *                            kernel ran and what it executes per evaluation, for the roofline in bench.py.
 *   fdg_graph_destroy, fdg_graph_query, fdg_last_error: lifetime / errors
 *                            (Julia exceptions in the reference, static.jl:6-11).
 *
 * Conventions: every function returns 0 on success and a negative FDG_E_* code
 * on failure; fdg_last_error() returns a thread-local message.  All buffers are
 * owned by the caller.  The program of a handle is immutable after create/specialize, and its
 * device scratch (spill panels, partial sums, staging buffers) is kept per caller stream, so the
 * device entry points may be called on one handle from several threads and on several streams at
 * once: calls on one stream run in stream order, calls on different streams may overlap on the
 * device.  (Enqueueing is serialised by a mutex inside the handle; up to 8 streams keep their
 * scratch, a ninth releases the least recently used set after a device synchronisation.  The first
 * call on a stream allocates; later ones only launch kernels, so they can be captured in a hipGraph.)
 * fdg_graph_specialize* and fdg_graph_release_device must not run concurrently with evaluations on
 * the same handle.  There is no CPU
 * fallback anywhere behind this ABI: device entry points fail with
 * FDG_E_NO_DEVICE when no gfx950 device is usable.
 *
 * Node table (value index space): leaves 0..n_leaf-1 in leafVal order, then
 * internal nodes n_leaf..n_leaf+n_node-1 in statement order; every child index
 * is smaller than its node's index.
 *
 * Arithmetic contract (what "identical results" means): fp64, no FMA
 * contraction, n-ary Sum/Prod evaluated as the left folds the reference's
 * generated code performs (static.jl:13-31 + Julia's left-associative n-ary
 * + and *):  Sum  = (((c1[*f1]) + (c2[*f2])) + ...),
 *            Prod = ((((c1[*f1]) * c2)[*f2]) * ...),
 *            Power{2} = c*c, Power{3} = c*c*c, other N = fdg_powi(c, N),
 * a factor is applied only when it differs from 1 (static.jl:15,18,25,28).
 */
#ifndef FDG_H
#define FDG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDG_VERSION 102 /* 0.1.1: tile-major batches, interpreter association */

#define FDG_OP_SUM 0u
#define FDG_OP_PROD 1u
#define FDG_OP_POWER 2u
#define FDG_NO_ROOT 0xFFFFFFFFu /* root id not present in any graph: root[k] left untouched */

enum {
  FDG_OK = 0,
  FDG_E_INVALID = -1,    /* malformed table / bad argument */
  FDG_E_UNSUPPORTED = -2,/* unknown operator (static.jl:6-11) */
  FDG_E_NO_DEVICE = -3,  /* no usable gfx950 device / HIP runtime failure */
  FDG_E_NOMEM = -4,
  FDG_E_JIT = -5,        /* kernel specialization failed */
  FDG_E_INTERNAL = -6
};

typedef struct fdg_graph_desc {
  uint32_t n_leaf;            /* L */
  uint32_t n_node;            /* N internal nodes */
  uint32_t n_root;            /* R */
  uint32_t n_edge;            /* E = child_off[n_node] */
  const uint8_t *op;          /* [N] FDG_OP_* */
  const int32_t *power;       /* [N] exponent for FDG_OP_POWER, ignored otherwise */
  const uint32_t *child_off;  /* [N+1] */
  const uint32_t *child_idx;  /* [E] value index of each operand */
  const double *child_fac;    /* [E] subgraph_factors */
  const uint32_t *root_slot;  /* [R] value index written to root[k], or FDG_NO_ROOT */
} fdg_graph_desc;

typedef struct fdg_graph fdg_graph; /* opaque */

/* What the lowering did; all counts are per graph, not per sample. */
typedef struct fdg_graph_info {
  uint32_t n_leaf, n_node, n_root, n_edge;
  uint32_t n_live_node;     /* internal nodes reachable from a root */
  uint32_t n_live_leaf;     /* leaves reachable from a root */
  uint64_t flops_alg;       /* adds + mults + factor mults + power mults, reachable part */
  uint64_t bytes_alg;       /* 8*(L+R): algorithmic HBM bytes per evaluation */
  uint32_t max_live;        /* peak number of simultaneously live values (leaves on demand) */
  uint32_t n_slot_lds;      /* per-sample fp64 slots kept in LDS by the interpreter */
  uint32_t n_slot_mem;      /* per-sample fp64 slots kept in the HBM workspace panel */
  uint32_t n_ops;           /* micro-ops in the interpreter stream */
  int32_t specialized;      /* 1 when a straight-line kernel is loaded */
  uint32_t spec_vgpr, spec_lds_bytes, spec_scratch_bytes; /* of the specialized kernel */
} fdg_graph_info;

/* flags for fdg_graph_specialize */
#define FDG_SPEC_DEFAULT 0u
#define FDG_SPEC_KEEP_SOURCE 1u   /* leave the generated source next to the code object */
#define FDG_SPEC_FAST_MATH 2u     /* allow FMA contraction (compiler flag for HIP source; with FDG_SPEC_ISA a product used
                                   * once by a sum becomes v_fma_f64): NOT bit-exact -- within 1e-12 of the sums' term
                                   * scale -- and reported separately */
#define FDG_SPEC_AUTOTUNE 8u      /* with FDG_SPEC_ISA: pick the configuration by timing a few candidates on
                                     the device (needs one); the choice is remembered in the cache directory */
#define FDG_SPEC_ROW_MAJOR_COMPANION 16u /* keep the handle's current (FDG_SPEC_ISA) kernels and add the HIP-source ones next to
                                   * them; sample-major input (compile_Python's [B,L]: leaf stride 1) is then evaluated by the
                                   * companion, whose lanes read their own rows, instead of being transposed for the ISA
                                   * kernel.  Worth it below 16 leaves, where the ISA back end has no row-major variant of its own; same bits either way. */
#define FDG_SPEC_ISA 4u           /* optimizing back end: own scheduler + register allocator, gfx950
                                     assembly printed directly (one VALU instruction per fold step) */

const char *fdg_last_error(void);
int fdg_version(void);

/* Host-only: validates and lowers the table (dead-code elimination, slot
 * allocation, interpreter stream).  Needs no device. */
int fdg_graph_create(const fdg_graph_desc *desc, fdg_graph **out);
int fdg_graph_destroy(fdg_graph *g);
int fdg_graph_query(const fdg_graph *g, fdg_graph_info *info);

/* The reference has TWO evaluators of a graph, and they round differently:
 *   FDG_ASSOC_STATIC (default): the generated eval_graph! of Compilers.compile (src/backend/static.jl:13-46), the contract above;
 *   FDG_ASSOC_INTERP: the interpreter eval! (src/computational_graph/eval.jl:1-3,15-39), which the reference's examples and tests
 *     call (example/benchmark.jl:84-86):  Sum = sum(w_i * f_i), Prod = prod(w_i * f_i) = (((w1*f1) * (w2*f2)) * (w3*f3)) ...,
 *     Power{N} = w^N * f -- every operand is scaled by its factor BEFORE it enters the left fold (sum / prod over a generator
 *     are left folds).  Multiplying by a factor 1.0 leaves the bits alone, so the two differ exactly where a Prod has a factor
 *     other than +-1 on its second or a later operand: ((acc * w) * f) against (acc * (w * f)).
 * A handle evaluates with ONE of them, on every back end (interpreter, HIP source, ISA, cooperative, Monte-Carlo step); choose
 * before the first fdg_graph_specialize* call (FDG_E_INVALID afterwards).  Host-only. */
#define FDG_ASSOC_STATIC 0
#define FDG_ASSOC_INTERP 1
int fdg_graph_set_association(fdg_graph *g, int assoc);

/* Options of a handle.  The library never reads the process environment while it specialises or launches: the FDG_* variables an
 * installation may set (FDG_CACHE_DIR, FDG_CACHE_RO_DIR, FDG_CACHE_TRUST, FDG_LLVM_BIN, FDG_HIPCC, FDG_JIT, FDG_MC_ROUTE,
 * FDG_EVAL_CHUNK, FDG_MC_CHUNK, FDG_SM_CHUNK_MB, FDG_IGNORE_TUNED, FDG_LEAF_GENERIC, FDG_TUNE_VERBOSE, FDG_ISA_[NO_]POOL, FDG_ISA_[NO_]RL)
 * are copied ONCE per process, every handle starts with a copy, and a handle's behaviour is a function of its own options from then on.
 * fdg_graph_set_option changes one (value NULL: removes it) -- the same names, plus the variant selectors and tuning knobs the tests and dev
 * tools use (FDG_ISA_W2, FDG_ISA_COOP, FDG_COOP_WAVES, FDG_ISA_NO_FUSED_ACC, FDG_ROOT_SCRATCH_MB, ...).  Options that shape
 * a kernel must be set before the fdg_graph_specialize* call that builds it; options of the launch path (FDG_ISA_NO_*, FDG_*_CHUNK*,
 * FDG_ROOT_SCRATCH_*, FDG_ISA_WAVES_PER_CU, FDG_ISA_OVERSUB, FDG_ISA_MEM_WAVES, FDG_ISA_TILE_CLAIM) take effect with the next call: they are
 * parsed into the handle here, and between an evaluation entry point and hipModuleLaunchKernel nothing is looked up by name.
 * FDG_ISA_TILE_CLAIM = "1" / "0": launches of the root-writing one-wave kernels that the plan finds bound by memory always / never use
 * the twin whose waves claim their next run of tiles from a counter in the stream's workspace (fdg_isa_eval_cl / fdg_isa_eval_nt_cl: the
 * same bits, the waves stay together however long the launch) instead of walking tiles w, w + n, ...; unset, launches of 256 rounds and
 * more do.  fdg_kernel_info::last_launch tells which walk a call used.  (FDG_ISA_CLAIM_RUN, at specialisation: tiles per claim, 4.)
 * Thread-safe against
 * concurrent launches of the same handle (taken under the handle's mutex).  Names must start with "FDG_".  fdg_graph_get_option returns
 * the value (owned by the handle, valid until the option changes) or NULL.  No counterpart in the reference. */
int fdg_graph_set_option(fdg_graph *g, const char *name, const char *value);
const char *fdg_graph_get_option(const fdg_graph *g, const char *name);
/* The process defaults: what handles created AFTER the call start with, and what the entry points that take no handle see
 * (fdg_leaf_eval_device*: FDG_LEAF_GENERIC).  Initialised from the environment at first use (supported names only). */
int fdg_set_default_option(const char *name, const char *value);
const char *fdg_get_default_option(const char *name);   /* valid until the calling thread's fourth next call of this function */

/* What the specialised kernels of a handle execute per evaluation and which of them the last device call launched --
 * the figures a roofline needs (bench.py: executed fold steps against the fp64 issue peak, bytes against HBM) without
 * guessing on the host side which variant the library picked.  Counts are per sample (one lane); slot 0 = the evaluator
 * (fdg_isa_eval[_nt]), 1 = fused accumulation (fdg_isa_eval_acc[_nt]), 2 = the row-major variant (fdg_isa_eval_rm).
 * All zero for handles that are not specialised with FDG_SPEC_ISA.  No counterpart in the reference. */
#define FDG_LAUNCH_CLAIMED 0x80000000u
typedef struct fdg_kernel_info {
  char last_kernel[48];       /* name of the evaluator kernel the last device call on this handle launched ("" = none yet) */
  uint64_t n_valu[3];         /* vector-ALU fold steps executed per evaluation (after value numbering / recomputation) */
  uint32_t n_ld_leaf[3];      /* leaf loads from the input matrix (> n_live_leaf: leaves evicted and read again) */
  uint32_t n_panel[3];        /* loads + stores of the HBM workspace panel */
  uint32_t n_lds[3];          /* loads + stores of per-lane LDS slots */
  uint32_t waves_per_cu[3];   /* resident waves per CU the launch uses */
  uint32_t has_acc, has_rm, has_coop, rm_bufs;
  uint32_t has_pool;          /* the pooled cooperative variant (fdg_isa_eval_pool) is installed: full tiles of batches whose samples of a leaf are contiguous */
  uint32_t pool_fetch;        /* ... leaf fetches from memory per evaluation (>= the live leaves) */
  uint64_t pool_valu;         /* ... fold steps executed per evaluation, all waves together */
  uint32_t has_rl;            /* the linear row-major variant (fdg_isa_eval_rl) is installed: contiguous rows, full tiles */
  uint32_t last_launch;       /* bits 0-30: workgroups of the last launch of an evaluator kernel of the optimizing back end (0 = none yet);
                               * bit 31 (FDG_LAUNCH_CLAIMED): its waves claimed their tiles from a counter (FDG_ISA_TILE_CLAIM) -- the kernel
                               * launched was the `_cl` twin of the variant last_kernel names */
  uint64_t rl_valu;          /* ... fold steps it executes per evaluation */
} fdg_kernel_info;
int fdg_graph_kernel_info(fdg_graph *g, fdg_kernel_info *info);

/* Emits HIP source for a straight-line kernel of this graph (one lane = one
 * sample, values in VGPRs, compiler-managed overflow) and returns it as a
 * malloc'ed NUL-terminated string the caller frees with fdg_free.  Host-only. */
int fdg_graph_emit_source(const fdg_graph *g, unsigned flags, char **source);
void fdg_free(void *p);

/* JIT: emit + compile for gfx950 (hiprtc, else `hipcc --genco`) + cache the code
 * object in cache_dir (NULL: $FDG_CACHE_DIR or /tmp/fdg-cache).  The module is
 * loaded lazily on first device use, so this works without a device present
 * (cross-compile at build time, run on the GPU box). */
int fdg_graph_specialize(fdg_graph *g, const char *cache_dir, unsigned flags);

/* Tuning knobs of the FDG_SPEC_ISA back end; zero fields take the default. */
typedef struct fdg_opt_params {
  uint32_t n_reg;          /* fp64 values kept in VGPR pairs (<= 125) */
  uint32_t n_lds;          /* fp64 LDS slots per lane (<= 127) */
  uint32_t lookahead_lds;  /* prefetch distance, in ops, of LDS loads */
  uint32_t lookahead_mem;  /* prefetch distance, in ops, of workspace-panel (L2/HBM) loads */
  uint32_t lookahead_leaf; /* prefetch distance, in ops, of first-use leaf loads (HBM) */
  uint32_t n_acc;          /* AGPR pairs per lane used as a spill level (<= 124; 0 with two waves per SIMD) */
  uint32_t vn_window;      /* value numbering of identical fold steps: 0 default, 1 off, n > 1 window in ops */
  uint32_t fma;            /* fdg_graph_opt_program only: 1 = fuse products into sums like FDG_SPEC_FAST_MATH does */
  uint32_t remat_window;   /* > 0: the value of a cheap node that has not been read for this many ops is forgotten and computed
                            * again by its next consumer (same operations, same bits): arithmetic instead of spill traffic */
  uint32_t remat_cost;     /* ... "cheap" = at most this many fold steps of its own (default 4) */
} fdg_opt_params;

/* One op of the register-allocated program (for inspection and for host-side
 * checkers that replay it): kind 0 LD_LEAF r[d]=leaf[a], 1 LD_LDS r[d]=lds[a],
 * 2 LD_MEM r[d]=ws[a], 3 ST_LDS lds[d]=r[a], 4 ST_MEM ws[d]=r[a],
 * 5 MUL r[d]=(+-r[a])*(+-r[b]), 6 ADD, 7 MULC r[d]=(+-r[a])*imm, 8 ROOT root[d]=+-r[a],
 * 10 LD_ACC r[d]=acc[a], 11 ST_ACC acc[d]=r[a].  Programs of fdg_graph_mc_program also contain the leaf formulas'
 * 16 ADDC r[d]=(+-r[a])+imm, 17 EXP r[d]=exp(+-r[a]), 18 RCP r[d]=1/(+-r[a]),
 * 19 SEL r[d]= cond(+-r[c]) ? +-r[a] : +-r[b] (cond: x>0 if imm==0, x>=0 otherwise), 20 FIXZ r[d]= r[a]==0 ? imm : r[a],
 * 21 SELC r[d]= cond(+-r[a]) ? imm : -imm (x>0 if negb==0, x>=0 otherwise); their LD_LEAF reads input column a
 * (momentum components first, then times). */
typedef struct fdg_mop {
  uint8_t kind, nega, negb, negc;
  uint32_t d, a, b;
  double imm;
  uint32_t c, param;   /* param (programs of fdg_graph_mc_program): 0, or imm is a physical parameter the kernel takes as an argument
                        * -- 1: -kF^2, 2: beta, 3: -beta, 4: lambda -- and holds the value the program was built with;
                        * c: third source of kinds 14 FMA r[d]=(+-r[a])*(+-r[b])+(+-r[c]) and 15 FMAC r[d]=(+-r[a])*imm+(+-r[c]),
                        * which only FDG_SPEC_FAST_MATH programs contain */
} fdg_mop;

/* Optional scheduling hint for FDG_SPEC_ISA: group[n] (n < n_node) tags internal nodes that belong
 * together -- e.g. the Taylor coefficients that taylorexpansion! (src/utility.jl:105-135) derives from
 * one original node share that node's id.  Members of a group are evaluated together.  Only the order
 * of evaluation changes, never a value.  Pass NULL to clear. */
int fdg_graph_set_schedule_groups(fdg_graph *g, const uint32_t *group, uint32_t n_node);

/* Sets the parameters used by the next fdg_graph_specialize(..., FDG_SPEC_ISA). */
int fdg_graph_set_opt_params(fdg_graph *g, const fdg_opt_params *prm);
/* Runs scheduler + allocator and returns the op list (malloc'ed; fdg_free).  Host-only. */
int fdg_graph_opt_program(const fdg_graph *g, const fdg_opt_params *prm, fdg_mop **ops, uint64_t *n_ops,
                          uint32_t *n_reg_used, uint32_t *n_lds_used, uint32_t *n_mem_used, uint32_t *n_acc_used);

/* The program of wave `wave` (0..3) of the cooperative variant -- the four waves of a CU evaluate one 64-sample tile
 * together, each on its share of the graph, values crossing between waves through shared LDS slots (kinds 25 SEND
 * shared[d]=r[a], 26 RECV r[d]=shared[a], 27 BARRIER) -- for inspection and host-side replay.  info[8] (optional):
 * registers, private LDS slots, panel slots, AGPR pairs of this wave; shared slots, barriers per tile, hand-overs per
 * tile, fold steps computed by more than one wave.  Host-only.  FDG_E_UNSUPPORTED when the graph has no wide root sum. */
int fdg_graph_coop_program(const fdg_graph *g, const fdg_opt_params *prm, uint32_t wave, fdg_mop **ops, uint64_t *n_ops,
                           uint32_t *info);

/* The programs of the POOLED cooperative variant (fdg_isa_eval_pool): whole roots are dealt to the eight waves of a CU, and no wave
 * loads a leaf from memory into a register -- the tile's leaves are fetched into a shared LDS pool (kind 29 POOL_FETCH shared[d] =
 * leaf[a], readable from epoch (uint32)imm on; LDS-direct loads issued epochs ahead by the waves in turn) and read from there (kind 26).
 * For graphs whose one-wave kernels re-read their leaves (the vertex functions of example/benchmark.jl and example/benchmark_GV.jl).
 * info as for fdg_graph_coop_program, with info[6] = leaf fetches per tile.  Host-only.  FDG_E_UNSUPPORTED when the graph has fewer
 * than two roots per wave or the pool cannot hold what an epoch reads. */
int fdg_graph_pool_program(const fdg_graph *g, const fdg_opt_params *prm, uint32_t wave, fdg_mop **ops, uint64_t *n_ops,
                           uint32_t *info);

/* ---- element types other than Float64 -----------------------------------------------------------------------------
 * The function Compilers.compile returns is generic in eltype(leafVal) (the generated text has no type in it,
 * src/backend/static.jl:98-133); to_Cstr / compile_C map the weight types they know (static.jl:135-153: Float32, ComplexF32,
 * ComplexF64, ...).  fdg_graph_specialize_typed compiles a per-graph HIP-source kernel for one such type,
 * fdg_eval_device_typed evaluates with leaf and root buffers of that type (strides in elements; a complex element is the pair
 * (re, im), as in Julia and C).  What it computes is what the Julia function computes on Vector{T} arguments: the factors are
 * Float64 literals in the text, so a factor != 1 promotes a Float32 value to Float64 for the rest of its expression (Julia's
 * promotion rules are C++'s here), products and sums of values of the type stay in the type, Complex * Complex is
 * (ar br - ai bi, ar bi + ai br) without contraction, Complex * Real scales both components (base/complex.jl), and a root is
 * converted to the element type when stored.  Covered: Sum, Prod, Power{2}, Power{3} (other literal powers take type-specific
 * paths through Base.power_by_squaring: FDG_E_UNSUPPORTED).  No ISA back end for these types: they go through the
 * compiler-scheduled kernels (every BASELINE configuration is Float64).  FDG_DT_F64 forwards to the ordinary entry points. */
#define FDG_DT_F64 0
#define FDG_DT_F32 1
#define FDG_DT_C64 2
#define FDG_DT_C32 3
int fdg_graph_specialize_typed(fdg_graph *g, int dtype, const char *cache_dir, unsigned flags);
/* ComplexF64 rows.  fdg_graph_create_complex_view returns a NEW handle (the caller's to destroy) for the Float64 graph that is g's
 * graph on Complex{Float64} values spelled out on real and imaginary parts: leaves re_0, im_0, re_1, im_1, ... -- a row of a
 * row-major ComplexF64 [B, L] matrix read as 2 L doubles --, roots (re, im) of g's roots, every operation the one
 * base/complex.jl performs (z w = (zr wr - zi wi, zr wi + zi wr), z f = (re f, im f), + componentwise, z^2 = z z, z^3 = (z z) z)
 * in the association of the evaluator's own folds, so the ordinary Float64 entry points give the generic function's bits on
 * ComplexF64 arguments.  FDG_E_UNSUPPORTED for other powers.  fdg_graph_specialize_typed(g, FDG_DT_C64, dir, FDG_SPEC_ISA) builds such
 * a view inside g and specialises it with the optimizing back end; fdg_eval_device_typed then sends row-major batches
 * (leaf_leaf_stride == 1, root_root_stride == 1) through its in-place row-major kernel when it has one, everything else through
 * the per-type kernel. */
int fdg_graph_create_complex_view(const fdg_graph *g, fdg_graph **out);
int fdg_eval_device_typed(fdg_graph *g, int dtype, const void *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                          void *d_root, int64_t root_sample_stride, int64_t root_root_stride, int64_t n_sample, void *stream);
/* The Monte-Carlo step for these types: the integrand's `sum weight * root over samples` around the generic eval_graph!, fused so that
 * the roots never reach memory.  d_acc[k] += sum_b w_b x_k(b), where x_k(b) is the value fdg_eval_device_typed would have stored as
 * root k of sample b -- converted to the element type first -- widened to Float64; with d_acc2 (optional, NULL: not wanted)
 * d_acc2[k] += sum_b (w_b x_k(b))^2.  Float32: d_acc and d_acc2 hold R doubles.  ComplexF64 / ComplexF32: R (re, im) pairs of
 * doubles, a ComplexF64[R]; the weights are real, so the sums run per component, and d_acc2[k] is (sum (w re)^2, sum (w im)^2).
 * d_weight: Float64[n_sample], NULL = weight 1.  Both buffers are added to; entries of roots that do not exist (FDG_NO_ROOT) keep
 * their bits (the sign of a zero included) on the per-type kernel's route.  A lane past the batch skips its sample (no weight-0 term: an infinite root gives an infinite sum, not NaN).
 * The kernel, fdg_spec_typed_acc, has the body of fdg_spec_typed: Float64 sums in registers, a shuffle butterfly per wave, the four wave sums
 * added in wave order, one partial per block and component; then fdg_reduce_partials in block order: no float atomics, bitwise
 * reproducible for the same arguments on the same device.  ComplexF64 rows under fdg_eval_device_typed's condition (the view exists,
 * leaf_leaf_stride == 1, leaf_sample_stride >= L, n_sample >= 64, the doubled stride addressable) go through the view's
 * fdg_accumulate_device -- with d_acc2 its fdg_accumulate_device_moments, one bin.  fdg_kernel_info::last_kernel names the route:
 * the view's kernel followed by " (ComplexF64 rows)", or fdg_spec_typed_acc<Float32 | ComplexF64 | ComplexF32>.  No promise of equal
 * bits is made between the two routes, nor between calls with and without d_acc2.  FDG_DT_F64 forwards to fdg_accumulate_device,
 * with d_acc2 to fdg_accumulate_device_moments with no bins, n_bin 1, tile stride 0.  FDG_E_INVALID before any device work: null
 * handle, unknown dtype, n_sample < 0, a type fdg_graph_specialize_typed has not compiled, NULL d_acc, d_acc == d_acc2, NULL d_leaf
 * when the graph has leaves.  n_sample == 0 or a graph without roots: FDG_OK, nothing touched. */
int fdg_accumulate_device_typed(fdg_graph *g, int dtype, const void *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                const double *d_weight, double *d_acc, double *d_acc2, int64_t n_sample, void *stream);

/* Evaluate B samples, buffers in device memory.
 *   leaf value i of sample b : d_leaf[b*leaf_sample_stride + i*leaf_leaf_stride]
 *   root value k of sample b : d_root[b*root_sample_stride + k*root_root_stride]
 * (strides in elements).  compile_Python's row-major [B,L] / [B,R] is
 * (L,1)/(R,1); a Julia column-major B x L matrix is (1,B)/(1,B).
 * stream: hipStream_t (NULL = default stream).  Asynchronous.
 * Any strides and bases are accepted and give the same values.  Column-major matrices whose column stride is a
 * multiple of 16 elements and whose bases lie on 128-byte lines (hipMalloc'ed buffers, B a multiple of 16) take the
 * streaming form of the kernel (non-temporal accesses), 3-5 % faster on graphs bound by memory. */
int fdg_eval_device(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride,
                    int64_t leaf_leaf_stride, double *d_root, int64_t root_sample_stride,
                    int64_t root_root_stride, int64_t n_sample, void *stream);

/* Host-buffer convenience: row-major leaf[B,L] -> root[B,R]; H2D, eval, D2H,
 * synchronous.  Same in-place semantics as eval_graph!(root, leafVal). */
int fdg_eval(fdg_graph *g, const double *leaf, double *root, int64_t n_sample);

/* Same with strided host matrices (element strides as in fdg_eval_device): row-major [B, L] / [B, R]
 * (value stride 1) or column-major B x L / B x R -- what a Julia Matrix is: sample stride 1, value
 * stride >= n_sample.  The device copy keeps the host's orientation, so a Julia matrix reaches the
 * evaluator leaf-major without any transposition pass.  Leaves and roots may differ in orientation. */
int fdg_eval_strided(fdg_graph *g, const double *leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                     double *root, int64_t root_sample_stride, int64_t root_root_stride, int64_t n_sample);

/* d_acc[k] += sum_b weight[b] * root_k(b)   (d_weight may be NULL: weight 1).
 * Per-lane accumulators inside the evaluator (ISA back end) or fixed-shape block trees, then one partial per
 * wave / block and root summed in fixed order by a second kernel: deterministic for a given launch shape, no atomics.
 * d_acc must hold n_root doubles and be zeroed by the caller. */
int fdg_accumulate_device(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride,
                          int64_t leaf_leaf_stride, const double *d_weight, double *d_acc,
                          int64_t n_sample, void *stream);

/* ---- tile-major batches ------------------------------------------------------------------------------------------------
 * The layout the evaluator streams best, and the one a Monte-Carlo driver that owns its sample batch should allocate: samples
 * are grouped in tiles of FDG_TILE_SAMPLES = 64 (one wave), and a tile's block of the array is contiguous,
 *   leaf value i of sample b : d_leaf[(b / 64) * leaf_tile_stride + (b % 64) * leaf_sample_stride + i * leaf_leaf_stride]
 *   root value k of sample b : d_root[(b / 64) * root_tile_stride + (b % 64) * root_sample_stride + k * root_root_stride]
 * -- a Julia Array{Float64,3}(undef, 64, L, cld(B, 64)) is (sample, leaf, tile) strides (1, 64, 64 L); its roots
 * Array{Float64,3}(undef, 64, R, cld(B, 64)) are (1, 64, 64 R).  A wave then reads ONE contiguous block of 512 L bytes front to
 * back instead of 64 samples of each of L columns that lie B * 8 bytes apart: L concurrent address streams per wave become one,
 * and every page of the batch is touched by one wave, once (the leaf-major matrix of the headline runs 0.66-0.77
 * of the HBM roofline depending on where its pages landed; the tile-major batch does not show the two modes).  The buffers hold
 * cld(n_sample, 64) whole tiles; lanes of a last partial tile are neither read nor written.  A tile stride of 0 stands for
 * 64 * sample stride: the call is then exactly fdg_eval_device / fdg_accumulate_device on a strided matrix.  Same values,
 * bit for bit, as every other layout.  Needs a handle specialised with FDG_SPEC_ISA (FDG_E_UNSUPPORTED otherwise).
 * Stands in for: eval_graph!(root, leafVal) once per sample (static.jl:100,131), as fdg_eval_device does. */
#define FDG_TILE_SAMPLES 64
int fdg_eval_device_tiled(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                          int64_t leaf_tile_stride, double *d_root, int64_t root_sample_stride, int64_t root_root_stride,
                          int64_t root_tile_stride, int64_t n_sample, void *stream);
int fdg_accumulate_device_tiled(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                int64_t leaf_tile_stride, const double *d_weight, double *d_acc, int64_t n_sample, void *stream);
/* Binned accumulation: the `measure` step of a Monte-Carlo integrand whose observable is a function of an
 * external variable.  For every sample b with 0 <= j = d_bin[b] - bin_base < n_bin:
 *     d_acc[j * R + k] += w[b] * root_k(b)          (w = d_weight[b], or 1 when d_weight is NULL)
 * Samples whose bin falls outside [0, n_bin) add nothing.  d_acc holds n_bin x R doubles, bin-major
 * (a Julia R x n_bin Matrix{Float64}; torch [n_bin, R]), and is added to, not overwritten.
 * bin_base: 0 for C / Python indices, 1 for Julia's 1-based ones.
 * Leaves as in fdg_eval_device_tiled: leaf_tile_stride 0 = a plain strided matrix (any back end);
 * != 0 = a tile-major batch (needs FDG_SPEC_ISA, FDG_E_UNSUPPORTED otherwise).  d_bin and d_weight are
 * plain vectors indexed by the sample number b in both cases.
 * Roots that do not exist (FDG_NO_ROOT) leave their column of every bin untouched.
 * No float atomics anywhere: bitwise reproducible for the same arguments on the same device.
 * 1 <= n_bin <= FDG_BIN_MAX (FDG_E_INVALID for 0, FDG_E_UNSUPPORTED above).
 * The roots of a chunk of samples (FDG_ROOT_SCRATCH_MB) go through the handle's column-major root scratch -- the same
 * route and the same bits as fdg_eval_device --, a deterministic pass bins them (csrc/fdg_binned.hip). */
#define FDG_BIN_MAX 16384
int fdg_accumulate_device_binned(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride,
                                 int64_t leaf_leaf_stride, int64_t leaf_tile_stride,
                                 const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                 const double *d_weight, double *d_acc, int64_t n_sample, void *stream);
/* Second moments, for Monte-Carlo error bars: fdg_accumulate_device_binned plus, with t = w[b] * root_k(b),
 *     d_acc2[j * R + k] += t * t                    (the square rounded to double before it is added)
 * d_acc comes out bit for bit as fdg_accumulate_device_binned leaves it for the same arguments (the same
 * chunks, segments and order of sums); d_acc2 is bitwise reproducible too.  Both arrays hold n_bin x R doubles
 * and are added to; FDG_NO_ROOT columns stay untouched in both.  d_bin == NULL: every sample is in bin 0,
 * n_bin must be 1 and bin_base is ignored (the plain sum with its error bar; the same bits as an all-zero d_bin).
 * FDG_E_INVALID: d_acc or d_acc2 NULL, d_acc == d_acc2, d_bin NULL with n_bin != 1, and the binned call's cases;
 * FDG_E_UNSUPPORTED: n_bin > FDG_BIN_MAX, or a tile-major batch without FDG_SPEC_ISA.  All before any device work. */
int fdg_accumulate_device_moments(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                  int64_t leaf_tile_stride, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                  const double *d_weight, double *d_acc, double *d_acc2, int64_t n_sample, void *stream);

/* harness: fdg_fill_uniform_device's values (same counters: sample_offset + b, i) written into a tile-major batch */
int fdg_fill_uniform_device_tiled(double *d_leaf, int64_t n_sample, uint32_t n_leaf, int64_t leaf_sample_stride,
                                  int64_t leaf_leaf_stride, int64_t leaf_tile_stride, uint64_t seed, uint64_t sample_offset,
                                  void *stream);

/* A matrix in one of the reference's layouts -> the tile-major batch, and back (round 6).  d_tiled is (64, n_col, cld(n_sample, 64)) as
 * fdg_eval_device_tiled takes it; the matrix is m[b * sample_stride + c * col_stride]: a Julia column-major B x C Matrix{Float64} is
 * (1, B) -- its 512-byte runs are copied as they are --, compile_Python's row-major [B, C] is (C, 1) -- 64 x 64 tiles through LDS.  One pass
 * at copy speed (read + written 5-6 TB/s): 2.3 x the time of ONE evaluation of the headline graph over the same batch, so it pays for a
 * batch that is evaluated several times, or when the producer of the leaves cannot write tile-major itself (fdg_leaf_eval_device_tiled
 * and the fused Monte-Carlo step do); DESIGN.md 6f has the measured cost.  Lanes past n_sample of the last tile are not written.
 * Stands in for nothing in the reference (its batched layout is compile_Python's [B, L], compiler_python.jl:23,28,45-47); the Julia shim
 * exposes them as tile_major!(dst, src) / from_tile_major!(dst, src). */
int fdg_repack_tile_major(const double *d_src, int64_t sample_stride, int64_t col_stride, double *d_tiled, int64_t n_sample,
                          uint32_t n_col, void *stream);
int fdg_unpack_tile_major(const double *d_tiled, double *d_dst, int64_t sample_stride, int64_t col_stride, int64_t n_sample,
                          uint32_t n_col, void *stream);

/* Device memory for a sample batch, backed explicitly (HIP virtual-memory management: one reserved address range, physical
 * chunks of chunk_bytes created and mapped in address order; chunk_bytes 0 = one physical allocation for the whole batch) instead
 * of by whatever state the driver's allocator is in when hipMalloc is called -- how a batch of tens of GB is backed decides
 * which of two rates its stream runs at.  The pointer is an ordinary device pointer for every entry point above and
 * for the caller's own kernels; release it with fdg_batch_free (synchronises the device).  The current device is used.
 * No counterpart in the reference (its leaf vector is a Julia Vector on the host). */
int fdg_batch_alloc(size_t bytes, size_t chunk_bytes, void **d_ptr);
int fdg_batch_free(void *d_ptr);

/* The two arrays of a TILE-MAJOR batch of one handle -- leaves (64, L, T) and roots (64, R, T), T = cld(n_sample, 64), strides as in
 * fdg_eval_device_tiled -- backed so that the evaluation streams at its fast rate over every part of the batch, whatever state the
 * driver's allocator is in (round 5).  On MI355X the rate at which a piece of leaves is evaluated depends on the physical
 * pages under that piece AND under the roots it writes: device memory falls into regions of two kinds, and reading one kind while writing
 * the same kind runs 10-12 % slower than the mixed combination (fused accumulation, which writes no roots, does not care).  Physical
 * addresses are invisible to a process; the rate is not.  With FDG_BATCH_PAIR_CALIBRATE the allocator maps the leaves in chunks of about
 * chunk_bytes_hint (0: 2 GB; rounded so that a chunk holds whole tiles of both arrays in whole mapping granules), draws more root chunks
 * than it needs -- from an 80 GB span of the device memory, or as much of it as is free beyond what the batch itself needs --, times the
 * handle's own evaluator on (leaf chunk, root chunk) pairs -- about a millisecond per pair -- and maps behind every leaf chunk the fastest
 * unused root chunk, drawing more while even the best is more than 3.5 % below the best pair seen (three levels were measured: 0.855 /
 * 0.80 / 0.765 of 8 TB/s on the headline graph; nothing is assumed about their number); what it drew and did not use goes back to the
 * driver.  When memory is short the search shrinks instead of failing (info->level_reached).  Monte-Carlo callers that only ACCUMULATE
 * (fdg_accumulate_device_tiled: no root is written) gain nothing from the pairing -- 0.89 of 8 TB/s on any allocation -- and should skip the
 * 7-9 s: allocate without the flag.  Without the flag the chunks are mapped in the order they were drawn (the A/B case).  Both arrays hold whole chunks (>= the T tiles asked for); release each with
 * fdg_batch_free.  `info` (may be NULL) reports what was found.  Needs a handle specialised with FDG_SPEC_ISA and the current device.
 * No counterpart in the reference (its leaf vector and root vector are Julia Vectors on the host, static.jl:100,131). */
#define FDG_BATCH_PAIR_CALIBRATE 1u
#define FDG_BATCH_PAIR_VERBOSE 2u   /* what the search saw, a few lines on stderr */
#define FDG_BATCH_PAIR_LEAF_MAJOR 16u /* the arrays are a Julia column-major pair B' x L and B' x R (strides (1, B'), B' = the mapped sample count: info->chunk_tiles * 64):
                                       * one window -- the whole batch --, the candidates are whole root matrices; pays while the leaf matrix lies in one or
                                       * two regions of the memory (up to a few tens of GB) */
#define FDG_BATCH_PAIR_ROW_MAJOR 8u /* the arrays are compile_Python's row-major [B, L] and [B, R] (compiler_python.jl:23,28,45-47) instead of the
                                     * tile-major ones: 64 consecutive rows take the place of a tile; everything else is the same */
typedef struct fdg_batch_pair_info {
  uint64_t leaf_bytes, root_bytes;   /* mapped bytes of the two arrays */
  uint64_t chunk_tiles;              /* 64-sample tiles per chunk */
  uint32_t n_chunk;                  /* chunks per array */
  uint32_t n_candidate;              /* root chunks drawn */
  uint32_t n_filler;                 /* 2 GB allocations held for a while to make the driver hand out other regions (released) */
  uint32_t n_probe;                  /* timed (leaf chunk, root chunk) pairs */
  uint32_t n_matched;                /* chunk pairs within 5 % of the best pair timed, as mapped */
  uint32_t calibrated;               /* 1: the candidates differed by more than 5 % (there was something to choose); 0: calibration off or no contrast */
  double gbs_fast, gbs_slow;         /* the best and the worst pair timed (algorithmic GB/s of one chunk's launch); "fast level" = within 3.5 % of gbs_fast */
  double gbs_before_mean, gbs_before_min;   /* chunk pairs as an uncalibrated mapping would have made them */
  double gbs_after_mean, gbs_after_min;     /* chunk pairs as mapped */
  double seconds;                    /* wall time of the call */
  double seconds_settling;           /* ... of which: waiting for the driver's background wipe of released memory to end */
  uint32_t level_reached;            /* how far the search got (round 6: it degrades, it does not fail, when memory is short).  0: no calibration (not asked
                                      * for, or windows too small to time); 1: asked for, but the leaves only fitted once every candidate had been given
                                      * back: mapped in draw order; 2: calibrated over a span of the memory cut short by what was free (the best pairs
                                      * found within it); 3: the full search */
  uint32_t span_gb;                  /* GB of fillers the candidates were drawn behind (80 at first, up to 144 more while the best pair seen is below par) */
} fdg_batch_pair_info;
int fdg_batch_alloc_pair(fdg_graph *g, int64_t n_sample, size_t chunk_bytes_hint, unsigned flags, void **d_leaf, void **d_root,
                         fdg_batch_pair_info *info);
/* test hook (host only): the allocator's search on a MODEL of the memory -- regions of four kinds, three pair levels, noise, further candidates
 * only behind further draws (scenario 0 ... 3, csrc/fdg_batch.cpp); returns how many of n_window windows ended with a candidate of the
 * complementary kind, *n_probe = pairs "timed".  So that the search is tested where there is no device. */
int fdg_selftest_pair_search(uint64_t seed, uint32_t scenario, uint32_t n_window, uint32_t *n_probe);

/* d_leaf[b*ss + i*ls] = U[0,1) from Philox4x32-10, key = seed, counter =
 * (sample_offset + b, i): independent of launch geometry and of how samples
 * are sharded over GPUs. */
int fdg_fill_uniform_device(double *d_leaf, int64_t n_sample, uint32_t n_leaf,
                            int64_t leaf_sample_stride, int64_t leaf_leaf_stride, uint64_t seed,
                            uint64_t sample_offset, void *stream);

/* Checks a gfx950 assembly listing (e.g. the `.s` a FDG_SPEC_ISA | FDG_SPEC_KEEP_SOURCE specialisation leaves in the
 * cache directory) against the wait-state table the ISA emitter itself uses (csrc/fdg_isa.cpp: trans result -> VALU,
 * VALU write of SGPR/VCC -> VALU read / v_div_fmas / VMEM, VALU -> v_readlane, wide store data -> VALU overwrite).
 * Returns the number of violations (0 = clean), < 0 on error; *report (optional, fdg_free) lists the rules, the
 * violations and what was checked.  Host-only; no counterpart in the reference (its code generator emits Julia). */
int fdg_isa_check_hazards(const char *asm_text, char **report);

/* Harness only (bench.py's `roofline.measured_copy_gbs`): d_dst[0..n) = d_src[0..n), 16 bytes per lane,
 * n even, both pointers 16-byte aligned.  The box's own streaming ceiling next to the 8 TB/s spec
 * (the reference has no counterpart). */
int fdg_copy_device(double *d_dst, const double *d_src, int64_t n, void *stream);

/* Harness only (bench.py's `roofline.measured_read_gbs`): streams d_src[0..n) through the chip with non-temporal loads and writes nothing
 * (d_sink: one double, written only if the data sums to a value it cannot have).  The memory system's ceiling for a read stream --
 * the evaluator's traffic is 95 % reads -- which is above what a copy reaches.  No counterpart in the reference. */
int fdg_read_device(const double *d_src, int64_t n, double *d_sink, void *stream);

/* Harness only (bench.py's `roofline.clock_ghz`): enqueues ONE wave on `stream` that sleeps for `seconds` of wall time
 * (0 < seconds <= 30) and then writes d_ticks[0] = shader-clock ticks, d_ticks[1] = 100 MHz ticks that went by: launched on
 * a side stream next to the evaluator it reports the clock the chip sustained under that load (the graphs at the
 * compute/memory ridge run against the power budget: 1.8-1.9 GHz instead of 2.4).  8 VGPRs, no LDS: it shares a SIMD with
 * two 248-register evaluator waves.  No counterpart in the reference. */
int fdg_clock_probe_device(double seconds, int64_t *d_ticks, void *stream);

/* ---- leaf values on device (the caller's side of the path) ----------------
 * The per-sample leaf loop of the reference's example integrand (example/benchmark.jl:58-81):
 *   loops = K[:, 1:n_loop] * basis                       (FrontEnds.update, src/frontend/pool.jl:69-76)
 *   type 1 (fermionic G): tau = T[tau_out] - T[tau_in];  eps = |loops[:, loop_index]|^2 - kF^2;
 *                         leaf = green(tau, eps, beta)   (example/benchmark.jl:113-127) for order 0;
 *                         orders 1..5: green_derive (benchmark.jl:93-111) = (-1)^n/n! d^n/d eps^n of the
 *                         fermionic kernel.  The reference calls Lehmann.jl's kernelFermiT_dw* for these;
 *                         Lehmann.jl is not part of the reference checkout, so the definition is restated
 *                         (overflow-safe closed form) and pinned by high-precision vectors, not by
 *                         Lehmann.jl output.  Other orders: "not implemented!" like benchmark.jl:108
 *   type 2 (bosonic V):   invK = 1/(|q|^2 + lambda);     leaf = 8*pi/invK * (lambda*invK)^order
 *   type 0:               leaf left untouched
 * with the tables FrontEnds.leafstates returns (src/frontend/frontends.jl:178-232; indices 1-based as
 * in the reference).  Writes the leaf matrix the evaluator reads, so the Monte-Carlo loop
 * (K, T) -> leaves -> graph -> accumulate never leaves the device.  Transcendentals differ from the
 * host libm in the last ulp: parity for this entry point is 1e-13 relative, not bit-exact. */
typedef struct fdg_leaf_tables {
  uint32_t n_leaf, n_basis, n_loop, dim, n_tau;
  const int32_t *leaf_type;    /* [n_leaf] 0 / 1 / 2 */
  const int32_t *leaf_order;   /* [n_leaf] derivative order of that leaf's own kind */
  const int32_t *tau_in;       /* [n_leaf] 1-based index into T */
  const int32_t *tau_out;      /* [n_leaf] */
  const int32_t *loop_index;   /* [n_leaf] 1-based index into the loop basis */
  const double *basis;         /* [n_basis][n_loop] */
  double kF, beta, lambda;
} fdg_leaf_tables;

/* K element (sample b, loop j, component d): d_K[b*k_sample_stride + (j*dim + d)*k_comp_stride];
 * T element (b, i): d_T[b*t_sample_stride + i*t_comp_stride]; leaves as in fdg_eval_device. */
int fdg_leaf_eval_device(const fdg_leaf_tables *tab, const double *d_K, int64_t k_sample_stride,
                         int64_t k_comp_stride, const double *d_T, int64_t t_sample_stride,
                         int64_t t_comp_stride, double *d_leaf, int64_t leaf_sample_stride,
                         int64_t leaf_leaf_stride, int64_t n_sample, void *stream);

/* The same with TILE-MAJOR leaves (fdg_eval_device_tiled): sample b of leaf i is written to
 * d_leaf[(b / 64) * leaf_tile_stride + (b % 64) * leaf_sample_stride + i * leaf_leaf_stride], so that the Monte-Carlo loop
 * (K, T) -> leaves -> fdg_accumulate_device_tiled runs on the layout the evaluator streams fastest. */
int fdg_leaf_eval_device_tiled(const fdg_leaf_tables *tab, const double *d_K, int64_t k_sample_stride,
                               int64_t k_comp_stride, const double *d_T, int64_t t_sample_stride,
                               int64_t t_comp_stride, double *d_leaf, int64_t leaf_sample_stride,
                               int64_t leaf_leaf_stride, int64_t leaf_tile_stride, int64_t n_sample, void *stream);

/* Fused Monte-Carlo step (the integrand of example/benchmark.jl:58-87 in one kernel):
 * the leaves are worked out in registers from the sample's loop momenta K and times T with the formulas
 * of fdg_leaf_eval_device and fed straight into the graph, so the 8*L bytes per evaluation of the leaf
 * matrix never exist.  fdg_graph_specialize_fused JIT-compiles the kernel for (graph, tables) -- tables as
 * for fdg_leaf_eval_device, n_leaf equal to the graph's, leaves without a formula (type 0) are 1.0 like
 * leafstates' initial leafValue; needs no device -- then
 *   fdg_mc_eval_device       root[b][k]           (strides as in fdg_eval_device)
 *   fdg_mc_accumulate_device acc[k] += sum_b weight[b] * root_k(b)   (weight NULL = 1)
 * with K, T laid out as in fdg_leaf_eval_device.  The single kernel is compiler-scheduled (HIP source through
 * hiprtc) and right for graphs of up to a few thousand operations.  For larger graphs the same calls run the
 * specialised leaf kernel into a chunk of leaves owned by the handle and then the handle's own evaluator
 * (specialise it with FDG_SPEC_ISA first): fdg_graph_specialize_fused picks the route by graph size
 * (FDG_MC_ROUTE=fused|split overrides); the roots are the same bits on either route. */
int fdg_graph_specialize_fused(fdg_graph *g, const fdg_leaf_tables *tab, const char *cache_dir, unsigned flags);
/* The third route, taken for large graphs on a handle specialised with FDG_SPEC_ISA: ONE kernel of the optimizing
 * back end whose inputs are the sample's n_loop*dim momentum components and n_tau times; every leaf is a value
 * computed in registers from them at its first use (ops 16..21 of fdg_mop: add-constant, exp, reciprocal, selects),
 * scheduled and register-allocated together with the graph.  kF, beta, lambda are arguments of that kernel (four scalar
 * registers: -kF^2, beta, -beta, lambda), so one code object per (graph, tables) serves every parameter set.  K and T
 * are read in place when both are component-major (sample stride 1; any two column strides); sample-major input is
 * packed into such arrays first.  Leaves agree with fdg_leaf_eval_device within its stated
 * tolerance (own exp: range reduction + degree-11 polynomial), not bit for bit.  FDG_MC_ROUTE=isa|split overrides.
 * fdg_graph_mc_program returns that program for inspection / host-side replay (tab->kF, beta, lambda are used). */
int fdg_graph_mc_program(const fdg_graph *g, const fdg_leaf_tables *tab, const fdg_opt_params *prm, fdg_mop **ops, uint64_t *n_ops,
                         uint32_t *n_reg_used, uint32_t *n_lds_used, uint32_t *n_mem_used, uint32_t *n_acc_used);
int fdg_mc_eval_device(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride, const double *d_T,
                       int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta, double lambda,
                       double *d_root, int64_t root_sample_stride, int64_t root_root_stride, int64_t n_sample, void *stream);
int fdg_mc_accumulate_device(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride, const double *d_T,
                             int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta, double lambda,
                             const double *d_weight, double *d_acc, int64_t n_sample, void *stream);
/* fdg_accumulate_device_binned for the fused Monte-Carlo step (K, T, kF, beta, lambda as in fdg_mc_accumulate_device;
 * every route: fused, split, one-kernel ISA). */
int fdg_mc_accumulate_device_binned(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                    const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride,
                                    double kF, double beta, double lambda,
                                    const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                    const double *d_weight, double *d_acc, int64_t n_sample, void *stream);
/* fdg_accumulate_device_moments for the fused Monte-Carlo step (every route; FDG_E_INVALID before
 * fdg_graph_specialize_fused). */
int fdg_mc_accumulate_device_moments(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                     const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride,
                                     double kF, double beta, double lambda,
                                     const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                     const double *d_weight, double *d_acc, double *d_acc2, int64_t n_sample, void *stream);

/* ---- VEGAS importance sampling (the front of the Monte-Carlo chain: where the samples and their weights come from) ----------------
 * The reference's examples and tests hand their integrand to MCIntegration (example/benchmark.jl:46-51, test/ver4.jl:224-237), whose
 * default solver is VEGAS: a separable piecewise-linear map per integration variable, refined between iterations from a histogram of
 * (f * jacobian)^2 per variable and grid cell.  MCIntegration is not part of the reference checkout: no counterpart in the reference;
 * the caller side of example/benchmark.jl:46-51.  One iteration = sample through a fixed map, evaluate, accumulate (estimate, error
 * bar, training histogram), all on the device; fdg_vegas_refine then moves the map on the host (D * G numbers).
 *
 * The map is a caller-owned array grid[d * (G + 1) + i], 0 <= d < D = n_dim, 0 <= i <= G = n_grid: the G + 1 cell edges of variable d
 * in physical units, strictly increasing.  1 <= D <= FDG_VEGAS_DIM_MAX, 1 <= G <= FDG_VEGAS_GRID_MAX (FDG_E_INVALID for 0,
 * FDG_E_UNSUPPORTED above, in every call below, before any device work).
 *
 * fdg_vegas_sample_device: for sample b < n_sample and variable d, every operation one rounded fp64 operation,
 *     u   = what fdg_fill_uniform_device writes for counter (sample_offset + b, d) and key seed (the same 53 bits)
 *     y   = u * G,  c = min((int)y, G - 1),  fr = y - c,  wd = grid[d][c + 1] - grid[d][c]
 *     x   = grid[d][c] + fr * wd        -> d_x[b * x_sample_stride + col[d] * x_col_stride]     (col NULL: col[d] = d)
 *     jac = (..((G * wd_0) * (G * wd_1)) * ..)   -> d_jac[b]       (left fold over d: the weight 1/pdf of the sample)
 *     c   -> d_cell[d * n_sample + b]   when d_cell is given (inspection; the accumulate calls do not need it)
 * d_grid is the map in device memory; col a HOST array of n_dim column numbers.  Columns of d_x that col does not name are not touched
 * (fixed external momenta, T[1] = 0 stay where they are); component-major x (sample stride 1) is what the one-kernel Monte-Carlo route
 * reads in place.  The result is a function of the arguments only (counter-based: independent of launch shape and of how samples are
 * sharded -- a rank passes the start of its range as part of sample_offset).  G = 1 on [0, 1] gives fdg_fill_uniform_device's bits and jac = 1. */
#define FDG_VEGAS_DIM_MAX 64
#define FDG_VEGAS_GRID_MAX 1024
int fdg_vegas_sample_device(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint64_t seed,
                            uint64_t sample_offset, double *d_x, int64_t x_sample_stride, int64_t x_col_stride, double *d_jac,
                            int32_t *d_cell, int64_t n_sample, void *stream);
/* The accumulate step of an iteration.  d_acc[k], d_acc2[k] (n_root doubles each, added to): bit for bit what
 * fdg_accumulate_device_moments / fdg_mc_accumulate_device_moments leave for the same arguments with d_bin = NULL, n_bin = 1 (the same
 * chunks, plan and pass): the estimate and its error bar.  d_hist[d * n_grid + c] (n_dim x n_grid doubles, added to) is the training
 * histogram: for every sample b, with c the cell of variable d recomputed from the Philox counter (sample_offset + b, d) exactly as the
 * sampler computes it (no cell array is read),
 *     s = (c_k0 * r_k0) + (c_k1 * r_k1) + ...   over the roots that exist, ascending k, left fold; the factor only when coef != NULL
 *     t = w_b * s   (d_weight NULL: t = s);   d_hist[d][c] += t * t
 * coef is a HOST array of n_root factors: the combination of roots the map is trained on (NULL: their plain sum).  seed,
 * sample_offset, n_dim, n_grid are the sampler's.  No float atomics: d_hist is bitwise reproducible for the same arguments on the same
 * device, and the order of every sum depends on (n_sample, n_dim, n_grid, n_root, FDG_ROOT_SCRATCH_MB) only; lanes past n_sample are
 * selected away, never multiplied by zero.  One more pass over the chunk's root scratch after the moments pass (csrc/fdg_binned.hip,
 * DESIGN.md 8b).  FDG_E_INVALID: d_acc, d_acc2 or d_hist NULL, any two of them the same buffer, the moments calls' cases, n_dim or
 * n_grid 0; FDG_E_UNSUPPORTED: the map's limits exceeded, a tile-major batch without FDG_SPEC_ISA; the Monte-Carlo form returns
 * FDG_E_INVALID before fdg_graph_specialize_fused.  All before any device work. */
int fdg_accumulate_device_vegas(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                int64_t leaf_tile_stride, const double *d_weight, const double *coef, uint64_t seed,
                                uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                int64_t n_sample, void *stream);
int fdg_mc_accumulate_device_vegas(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride, const double *d_T,
                                   int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta, double lambda,
                                   const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                   uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, int64_t n_sample, void *stream);
/* Lepage's refinement of the map from a training histogram (both HOST arrays; host only), per variable, in fp64, in this order:
 *  1. h = hist[d].  sum(h) <= 0 or G == 1: the variable is left alone.  A negative or non-finite entry anywhere: FDG_E_INVALID.
 *  2. smooth: s_0 = (7 h_0 + h_1) / 8, s_{G-1} = (h_{G-2} + 7 h_{G-1}) / 8, s_i = (h_{i-1} + 6 h_i + h_{i+1}) / 8; s /= sum(s).
 *  3. damp: w_i = ((1 - s_i) / (-log s_i))^alpha for 0 < s_i < 1, 0 for s_i = 0, 1 for s_i = 1.
 *  4. rebin: the new interior edge i (1 .. G - 1) lies where the running sum of w reaches i * sum(w) / G, linearly inside the old cell
 *     it falls in; the two end edges are copied bit for bit.
 *  5. the result is strictly increasing, or FDG_E_INTERNAL is returned.
 * alpha in [0, 2] (0: the grid comes back unchanged; FDG_E_INVALID outside).  On any error the grid is untouched. */
int fdg_vegas_refine(double *grid, const double *hist, uint32_t n_dim, uint32_t n_grid, double alpha);

/* ---- A discrete external variable for VEGAS, and binned observables --------------------------------------------------------------
 * The reference integrates its vertex function over (K, T, ExtKidx) with ExtKidx = MCIntegration.Discrete(1, Nk): the variable picks one
 * of Nk external-momentum configurations, the external legs are looked up from it, the observable is one estimate per configuration,
 * and the variable's probabilities are trained like the continuous map (test/ver4.jl:221-250; example/strong_coupling_expansion/).
 * MCIntegration is not part of the reference checkout: no counterpart in the reference; the caller's side of test/ver4.jl:224-237.
 *
 * The variable has n_bin values, 1 <= n_bin <= FDG_BIN_MAX, a cumulative distribution cdf[0 .. n_bin] with cdf[0] == 0,
 * cdf[n_bin] == 1 exactly and strictly increasing (every value has probability > 0), and an optional table ext[n_bin][n_ext],
 * 0 <= n_ext <= FDG_VEGAS_EXT_MAX, of what the value means for the integrand: row j is copied into the columns ext_col[0 .. n_ext) of
 * the sample's x (the components of the external momenta).
 *
 * fdg_vegas_sample_device_discrete: for sample b < n_sample, every step one rounded fp64 operation,
 *     the continuous variables d < n_dim exactly as fdg_vegas_sample_device (the same x bits in the same columns, the same d_cell);
 *     jc = the value that call writes to d_jac[b]
 *     u  = the uniform of Philox counter (sample_offset + b, n_dim), key seed: the column behind the continuous ones, so adding the
 *          discrete variable moves no continuous sample
 *     j  = the number of interior edges cdf[1 .. n_bin - 1] that are <= u
 *     p  = cdf[j + 1] - cdf[j];   jc / p -> d_jac[b];   j + bin_base -> d_bin[b];   ext[j][e] -> d_x[b * x_sample_stride + ext_col[e] * x_col_stride]
 * d_cdf (n_bin + 1 doubles) and d_ext (n_bin x n_ext doubles, row-major) are device memory; ext_col a HOST array of n_ext column numbers;
 * n_ext == 0: d_ext and ext_col may be NULL.  n_bin == 1 gives fdg_vegas_sample_device's x and jac bit for bit and d_bin = bin_base.
 * FDG_E_INVALID: a NULL d_grid, d_cdf, d_x, d_jac or d_bin, n_sample < 0, n_dim, n_grid or n_bin 0, n_ext > 0 without d_ext or ext_col,
 * an ext_col that repeats or names a column of col; FDG_E_UNSUPPORTED: the limits exceeded.  All before any device work.  The result is
 * a function of the arguments only (counter-based), so shards reproduce the unsharded batch.  The cdf is not read on the host: what it
 * must satisfy is the caller's to keep (fdg_vegas_refine_discrete does).  Neither is the width of x an argument: that every column
 * col and ext_col name exists in d_x is the caller's to keep as well, as in fdg_vegas_sample_device. */
#define FDG_VEGAS_EXT_MAX 16
int fdg_vegas_sample_device_discrete(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const double *d_cdf,
                                     uint32_t n_bin, int32_t bin_base, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                     uint64_t seed, uint64_t sample_offset, double *d_x, int64_t x_sample_stride, int64_t x_col_stride,
                                     double *d_jac, int32_t *d_bin, int32_t *d_cell, int64_t n_sample, void *stream);
/* The accumulate step with the discrete variable: binned moments and the training of both maps in one pass over the roots (the roots
 * of a chunk are evaluated once).
 *   d_acc, d_acc2 (n_bin x n_root, added to): bit for bit what fdg_accumulate_device_moments / fdg_mc_accumulate_device_moments leave for
 *     the same d_bin, bin_base, n_bin, weights and samples.
 *   d_hist (n_dim x n_grid, added to): the continuous training histogram of fdg_accumulate_device_vegas over the samples whose bin lies
 *     in [bin_base, bin_base + n_bin); when every sample's does, bit for bit what that call leaves for the same arguments (its cut
 *     depends on n_root, not on n_bin).
 *   d_hist_bin (n_bin doubles, added to; NULL: the discrete variable is not trained): d_hist_bin[j] += t * t over the samples of bin j,
 *     t = w_b * ((c_k0 * r_k0) + (c_k1 * r_k1) + ...) exactly as fdg_accumulate_device_vegas forms it.
 * A sample whose bin is out of range adds nothing to any of the four (it enters no sum: selected away, never multiplied by zero).  No float atomics:
 * d_hist_bin is bitwise reproducible for the same arguments on the same device, and the order of its sums depends on (n_sample, n_bin,
 * n_dim, n_grid, n_root, FDG_ROOT_SCRATCH_MB) only.  Errors: those of the moments calls and of the VEGAS calls; any two
 * of the four output arrays the same buffer, d_bin NULL (use the call without a discrete variable): FDG_E_INVALID.  All before any
 * device work. */
int fdg_accumulate_device_vegas_binned(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                       int64_t leaf_tile_stride, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                       const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                       uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin,
                                       int64_t n_sample, void *stream);
int fdg_mc_accumulate_device_vegas_binned(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                          const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta,
                                          double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight,
                                          const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid,
                                          double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin, int64_t n_sample,
                                          void *stream);
/* The refinement of the discrete variable's probabilities from its training histogram (both HOST arrays; host only), in fp64, in this order:
 *  1. p_j = cdf[j + 1] - cdf[j].  A negative or non-finite histogram entry, alpha outside [0, 2], floor outside [0, 1), or a cdf that
 *     does not run 0 .. 1 strictly increasing: FDG_E_INVALID.
 *  2. q_j = hist_bin[j] * p_j; sum(q) (left fold) <= 0, alpha == 0 or n_bin == 1: the cdf comes back unchanged.
 *  3. s_j = q_j / sum(q);  w_j = s_j ^ alpha, 0 for s_j = 0.
 *  4. p'_j = ((1 - floor) * w_j) / sum(w) + floor / n_bin   (sum(w) a left fold).
 *  5. cdf' = the left-fold running sum of p', cdf'[0] = 0, cdf'[n_bin] = 1 exactly.
 *  6. cdf' is strictly increasing, or FDG_E_INTERNAL is returned.  On any error cdf is untouched.
 * The expected hist_bin[j] is N * I2_j / p_j with I2_j the integral of (f_j * jac_c)^2, so q_j is proportional to I2_j whatever the
 * current p: the iteration has one fixed point, at alpha = 1/2 p_j ~ sqrt(I2_j), which minimises the sum over the bins of the second
 * moments I2_j / p_j.  floor keeps every bin sampled (a bin with p = 0 would silently lose its estimate). */
int fdg_vegas_refine_discrete(double *cdf, const double *hist_bin, uint32_t n_bin, double alpha, double floor);

/* ---- Spherical momentum variables for VEGAS ---------------------------------------------------------------------------------------
 * The reference integrates its loop momenta as MCIntegration.FermiK(dim, kF, 0.2 kF, 10 kF) (example/benchmark.jl:46,
 * example/benchmark_GV.jl:47, test/ver4.jl:224): a vector with a modulus and a direction, over a ball with the measure
 * k^(dim-1) dk dOmega.  MCIntegration is not part of the reference checkout: no counterpart in the reference; the caller's side of those
 * lines.  Here a group of 2 or 3 consecutive VEGAS variables is read as (k, phi) or (k, theta, phi), and the sampler writes the
 * Cartesian components into the columns of x the evaluator reads; the map stays separable in the polar variables, which is what
 * follows a shell |K| ~ kF with one variable.
 *
 * Group g = polar[g] takes the variables var, var + 1 (dim 2: k, phi) or var, var + 1, var + 2 (dim 3: k, theta, phi) and writes
 * the columns col[0 .. dim).  fdg_vegas_sample_device_polar: for sample b < n_sample, every step one rounded fp64 operation, in this order,
 *   1. every variable d < n_dim exactly as fdg_vegas_sample_device draws it: v_d = grid[d][c] + fr * wd, jc the same left fold of
 *      G * wd_d over ALL d, the same d_cell entries.  A variable of no group: v_d -> column col[d] as there.  A variable of a group is
 *      written nowhere, and its col[d] is not read.
 *   2. the groups, in the order of the array:
 *        dim 3: (st, ct) = fdg_sincos(theta); (sp, cp) = fdg_sincos(phi); ks = k * st;
 *               ks * cp -> col[0], ks * sp -> col[1], k * ct -> col[2];   jc = jc * k; jc = jc * k; jc = jc * st
 *        dim 2: (sp, cp) = fdg_sincos(phi);   k * cp -> col[0], k * sp -> col[1];   jc = jc * k
 *   3. d_cdf != NULL: the discrete variable exactly as fdg_vegas_sample_device_discrete (Philox column n_dim, jc / p -> d_jac[b], the
 *      bin, the table's row).  d_cdf == NULL: no discrete variable; jc -> d_jac[b]; n_bin, bin_base, d_bin, d_ext, n_ext and ext_col are
 *      ignored and d_bin may be NULL.
 * n_polar == 0 gives the bits of fdg_vegas_sample_device (d_cdf NULL) or of fdg_vegas_sample_device_discrete.  polar is a HOST array.
 * The result is a function of the arguments only (counter-based), so shards reproduce the unsharded batch.  The training pass of
 * the accumulate calls recomputes a sample's cells from its Philox counters and never looks at x, so they serve unchanged with
 * n_dim = the number of VEGAS variables.
 * The edges live in device memory and are not read on the host: that k >= 0, theta lies in [0, pi] and phi in [0, 2 pi] (fdg_sincos'
 * domain; a weight carries sin theta, which is >= 0 on [0, fl(pi)]) is the caller's to keep.
 * FDG_E_INVALID: polar NULL with n_polar > 0, a dim that is not 2 or 3, var + dim > n_dim, two groups sharing a variable, a column
 * named twice among the col[d] of the variables of no group, the groups' columns and (with d_cdf) ext_col, and the cases of
 * fdg_vegas_sample_device / _discrete; FDG_E_UNSUPPORTED: n_polar > FDG_VEGAS_POLAR_MAX and those calls' limits.  All before any
 * device work. */
#define FDG_VEGAS_POLAR_MAX 21
typedef struct fdg_vegas_polar { uint32_t var, dim, col[3]; } fdg_vegas_polar;
int fdg_vegas_sample_device_polar(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const double *d_cdf,
                                  uint32_t n_bin, int32_t bin_base, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                  const fdg_vegas_polar *polar, uint32_t n_polar, uint64_t seed, uint64_t sample_offset, double *d_x,
                                  int64_t x_sample_stride, int64_t x_col_stride, double *d_jac, int32_t *d_bin, int32_t *d_cell,
                                  int64_t n_sample, void *stream);
/* The sine and cosine the sampler uses, for 0 <= x <= 2 pi (the double nearest above included): Cody-Waite reduction to a quadrant,
 * two Horner polynomials, selection; no FMA, the order of every operation and every constant in csrc/fdg_sincos.h, so a restatement
 * in numpy gives the same bits.  |s - sin x|, |c - cos x| <= 4 * 2^-53; s >= 0 on [0, fl(pi)].  Exposed so host-side checkers can
 * call the very same routine.  Pure host function. */
void fdg_sincos(double x, double *s, double *c);

/* ---- Projection of the roots onto Matsubara frequencies in the accumulate step -------------------------------------------------------
 * Every root of a self-energy or vertex graph carries its own pair of external times (extT_labels, example/benchmark.jl:26-31), which
 * are integration variables; the `measure` step of a real calculation multiplies root k by a phase of tau_k = T[t_out(k)] - T[t_in(k)]
 * before it sums -- phase(varT, ver4.Tpair[...]) of test/ver4.jl:193 -- and so obtains Sigma(i omega_n) or Gamma at given frequencies:
 * one complex number per root, frequency and external configuration.  That is the caller's side of test/ver4.jl:193 (the integrand
 * handed to MCIntegration): no counterpart in the reference checkout.
 *
 * fdg_matsubara_phase: (s, c) = (sin, cos) of omega_n tau, omega_n = (2n+1) pi / beta (fermionic != 0) or 2n pi / beta, n of either
 * sign; the convention is e^{+i omega_n tau} = c + i s (for the other sign pass -n, fermions: -n - 1).  Every line ONE rounded fp64
 * operation, no FMA, in this order (csrc/fdg_matsubara.h, shared by host and device; a numpy restatement gives the same bits):
 *     x  = tau / beta
 *     m  = x * (double)(fermionic ? 2n+1 : 2n)
 *     h  = m * 0.5;   fl = floor(h);   r = h - fl        (0 <= r <= 1)
 *     th = r * 6.283185307179586                         (inside fdg_sincos' domain, its top end included)
 *     (s, c) = fdg_sincos(th)
 * |s - sin|, |c - cos| <= (4 pi |2n+1| + 16) * 2^-53 for |tau| <= beta.  A bosonic n = 0 gives exactly (0, 1).  Pure host function.
 *
 * The accumulate calls: for every sample b whose bin j = d_bin[b] - bin_base lies in [0, n_bin) (d_bin NULL: every sample in bin 0,
 * n_bin must be 1), every root k that exists and every frequency f < n_freq,
 *     t   = w_b * root_k(b)                               (the moments call's term; d_weight NULL: t = root)
 *     tau = T[b][root_tau_out[k]] - T[b][root_tau_in[k]]
 *     (s, c) = fdg_matsubara_phase(tau, beta, freq[f], fermionic)
 *     tre = t * c;   tim = t * s
 *     d_acc_re [(j * n_freq + f) * R + k] += tre;         d_acc_im [..] += tim
 *     d_acc2_re[(j * n_freq + f) * R + k] += tre * tre;   d_acc2_im[..] += tim * tim      (squares rounded before they are added)
 * The four arrays hold n_bin x n_freq x n_root doubles each (torch [n_bin, n_freq, R]) and are added to; FDG_NO_ROOT columns stay
 * untouched in all four.  freq (n_freq int32), root_tau_in and root_tau_out (n_root int32 each, 1-based like fdg_leaf_tables) are HOST
 * arrays.  T element (b, i), i 1-based: d_T[b * t_sample_stride + (i - 1) * t_comp_stride], as fdg_leaf_eval_device addresses it.  In
 * the Monte-Carlo form a NULL d_T in the descriptor means the call's own T and strides.  beta is the descriptor's in both forms.
 *
 * Besides the descriptor each call takes what the _vegas_binned calls take, with more of it optional:
 *   d_bin       NULL: no discrete variable (n_bin 1, d_hist_bin must be NULL): the arguments of the calls without one.
 *   d_acc, d_acc2  both NULL: the unprojected moments are not wanted; both given: bit for bit what the moments calls leave.
 *   the training block  n_dim == 0 and d_hist == NULL: no training.  Otherwise d_hist (and d_hist_bin, when given) come out bit for
 *               bit as fdg_[mc_]accumulate_device_vegas[_binned] leave them for the same arguments: the training stays on the
 *               unprojected (w sum_k c_k r_k)^2 and its plan does not change.
 * The roots of a chunk are evaluated once for everything the call produces, through the handle's root scratch by the route of
 * fdg_eval_device / fdg_mc_eval_device (every back end, layout, association and Monte-Carlo route).  No float atomics; samples past
 * n_sample or with a bin out of range are selected away, never multiplied by zero; the order of every sum of the four arrays is a
 * function of (n_sample, n_bin, n_freq, n_root, FDG_ROOT_SCRATCH_MB) only, so the same arguments give the same bits (csrc/fdg_binned.hip,
 * DESIGN.md 8e).
 * FDG_E_INVALID: a NULL descriptor, freq, root_tau_in, root_tau_out, T or one of the four arrays; any two output arrays of the call
 * the same buffer; one of d_acc, d_acc2 without the other; n_freq == 0; beta <= 0; a time label of an existing root outside
 * [1, n_tau]; d_hist_bin without d_bin; the cases of the moments and VEGAS calls.  FDG_E_UNSUPPORTED: n_freq > FDG_MATSUBARA_FREQ_MAX,
 * n_bin * n_freq > FDG_BIN_MAX, and those calls' limits.  All before any device work. */
#define FDG_MATSUBARA_FREQ_MAX 64
typedef struct fdg_matsubara {
  uint32_t n_freq;             /* 1 .. FDG_MATSUBARA_FREQ_MAX */
  int32_t fermionic;           /* != 0: omega_n = (2n+1) pi / beta;  0: 2n pi / beta */
  const int32_t *freq;         /* HOST [n_freq]: the n of every frequency */
  const int32_t *root_tau_in;  /* HOST [n_root], 1-based index into T */
  const int32_t *root_tau_out; /* HOST [n_root] */
  double beta;
  const double *d_T;           /* device; NULL in the Monte-Carlo form: the call's T */
  int64_t t_sample_stride, t_comp_stride;
  uint32_t n_tau;
  double *d_acc_re, *d_acc_im, *d_acc2_re, *d_acc2_im;   /* device, [n_bin][n_freq][n_root] each */
} fdg_matsubara;
void fdg_matsubara_phase(double tau, double beta, int32_t n, int fermionic, double *s, double *c);
int fdg_accumulate_device_matsubara(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                    int64_t leaf_tile_stride, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                    const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                    uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin,
                                    const fdg_matsubara *mz, int64_t n_sample, void *stream);
int fdg_mc_accumulate_device_matsubara(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                       const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta,
                                       double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight,
                                       const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid,
                                       double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin, const fdg_matsubara *mz,
                                       int64_t n_sample, void *stream);

/* ---- Weight groups: per-root integration variables (MCIntegration's `dof`) --------------------------------------------------------------
 * A diagrammatic series is integrated with all its orders at once, and every order has its own number of loop momenta and times:
 * `dof = [[diagpara[o].totalTauNum - 1,] for o in 1:length(orders)]` (test/hubbard.jl:81-85), `dof = [[2, 2], [3, 3], ..., [9, 9]]`
 * (example/strong_coupling_expansion/naive.jl:195), the same argument with one entry in test/ver4.jl:233.  Integrand i is then
 * weighted by the jacobian of its own variables only, and every variable's map is trained by the integrands that use it.
 * MCIntegration is not part of the reference checkout: no counterpart in the reference; the caller's side of those lines.
 *
 * Roots are assigned to groups and every group owns a set of the VEGAS variables: root k belongs to group root_group[k], bit d of
 * var_mask[g] says that variable d belongs to group g, and the weight of group g for sample b is d_weight[g * weight_group_stride + b]
 * (torch [n_group, n_sample]: stride n_sample).  root_group and var_mask are HOST arrays.
 *
 * fdg_vegas_sample_device_grouped: the arguments of fdg_vegas_sample_device_polar plus (var_mask, n_group, jac_group_stride).  x,
 * d_bin, d_cell and the table's row come out bit for bit as that call writes them; every variable is drawn once.  For sample b and
 * group g, every step one rounded fp64 operation, in this order,
 *   1. j_g = the left fold, over ascending d with bit d in var_mask[g], of G * wd_d; an empty mask gives 1.0;
 *   2. the polar groups, in the order of the array, whose variables belong to the mask: dim 3: j_g = j_g * k; * k; * st;  dim 2: j_g * k;
 *   3. d_cdf != NULL: j_g / p (the discrete variable is shared by every group);
 *   j_g -> d_jac[g * jac_group_stride + b].
 * A group whose mask holds all n_dim variables reproduces the bits of fdg_vegas_sample_device_polar's d_jac.
 * FDG_E_INVALID: var_mask NULL, n_group == 0, a mask bit at or above n_dim, a mask that holds some but not all variables of a polar
 * group, jac_group_stride < n_sample with n_group > 1, and the cases of fdg_vegas_sample_device_polar; FDG_E_UNSUPPORTED:
 * n_group > FDG_WEIGHT_GROUP_MAX and that call's limits.  All before any device work.
 *
 * fdg_[mc_]accumulate_device_grouped: the arguments of the _matsubara calls, where mz may now be NULL (no projection), plus wg.
 * With g(k) = root_group[k] and w_g = d_weight[g * weight_group_stride + b]:
 *   moments, binned moments and the projection: t = w_g(k) * root_k(b) wherever those calls form w_b * root_k(b); nothing else changes.
 *   continuous training: for every group with a root that exists, s_g = the left fold over its existing roots, ascending k, of
 *       c_k * r_k (the factor only with coef != NULL);  q_g = (w_g * s_g)^2, the product and the square each rounded;
 *       d_hist[d][c] += v_d, v_d the left fold, over ascending g with bit d in var_mask[g] and a root that exists, of q_g.  A variable
 *       of no such group is not added to at all.
 *   discrete training: d_hist_bin[j] += the left fold of q_g over all groups that have a root that exists, ascending g.
 * With n_group == 1, root_group all zero and a full mask every output carries the bits of the corresponding ungrouped call for the
 * same arguments (_moments, _vegas, _vegas_binned, _matsubara): the same kernels on the same plan.  With several groups: no float
 * atomics; samples past n_sample or out of range are selected away, never multiplied by zero; the order of every sum is a function of
 * (n_sample, n_bin, n_freq, n_root, n_dim, n_grid, n_group, FDG_ROOT_SCRATCH_MB) only, not of the masks or of root_group
 * (csrc/fdg_binned.hip).
 * FDG_E_INVALID: wg or one of its arrays NULL, d_weight NULL, n_group == 0, root_group[k] >= n_group for a root that exists, a mask
 * bit at or above n_dim when training is asked for, weight_group_stride < n_sample with n_group > 1, and the cases of the _matsubara
 * calls except the NULL descriptor (without one: those of the VEGAS calls with a training block, else of the moments calls);
 * FDG_E_UNSUPPORTED: n_group > FDG_WEIGHT_GROUP_MAX and those calls' limits.  All before any device work. */
#define FDG_WEIGHT_GROUP_MAX 8
typedef struct fdg_weight_groups {
  uint32_t n_group;             /* 1 .. FDG_WEIGHT_GROUP_MAX */
  const uint32_t *root_group;   /* HOST [n_root]: the group of root k (ignored for FDG_NO_ROOT roots) */
  const uint64_t *var_mask;     /* HOST [n_group]: bit d set = VEGAS variable d belongs to the group (D <= 64 = FDG_VEGAS_DIM_MAX) */
  int64_t weight_group_stride;  /* weight of group g, sample b: d_weight[g * weight_group_stride + b] */
} fdg_weight_groups;
int fdg_vegas_sample_device_grouped(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const double *d_cdf,
                                    uint32_t n_bin, int32_t bin_base, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                    const fdg_vegas_polar *polar, uint32_t n_polar, const uint64_t *var_mask, uint32_t n_group,
                                    int64_t jac_group_stride, uint64_t seed, uint64_t sample_offset, double *d_x, int64_t x_sample_stride,
                                    int64_t x_col_stride, double *d_jac, int32_t *d_bin, int32_t *d_cell, int64_t n_sample, void *stream);
int fdg_accumulate_device_grouped(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                  int64_t leaf_tile_stride, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight,
                                  const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc,
                                  double *d_acc2, double *d_hist, double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg,
                                  int64_t n_sample, void *stream);
int fdg_mc_accumulate_device_grouped(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride, const double *d_T,
                                     int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta, double lambda,
                                     const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight, const double *coef,
                                     uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2,
                                     double *d_hist, double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg,
                                     int64_t n_sample, void *stream);

/* ---- Observables: linear combinations of the roots, with their covariance ----------------------------------------------------------------
 * What a caller reports is rarely a root: the reference's own measurement sums a vertex function's roots into a direct and an exchange
 * component per external configuration (test/ver4.jl:184-216, `obs = zeros(Nk, 2)`), a self-energy series is summed over its orders.
 * All roots of a run are evaluated on the same samples, so the error bar of a sum, a difference or a ratio of roots cannot be formed
 * from the per-root d_acc2: it needs the covariance.  MCIntegration is not part of the reference checkout: no counterpart in the
 * reference; the caller's side of those lines.
 *
 * fdg_[mc_]accumulate_device_observables: the arguments of the _grouped calls plus ob.  Every optional block stays optional in the same
 * way (the bin vector, d_acc / d_acc2, the training block, d_hist_bin, mz); wg may be NULL (one weight column d_weight[b], or no
 * weights with d_weight == NULL); d_acc and d_acc2 may both be NULL.  coef is a HOST array, row-major [n_obs][n_root].
 * For every sample b < n_sample whose bin j is in range, every step one rounded fp64 operation:
 *   t_k = w_g(k) * root_k(b), as the moments pass forms it (root_k(b) without weights);
 *   o_m = the left fold of coef[m][k] * t_k over ascending k, over the roots that exist with coef[m][k] != 0.0; the first product
 *         starts the fold (no 0.0 + in front).  A row without a term contributes nothing: its column of d_obs and its rows and
 *         columns of d_cov are left untouched, as the columns of FDG_NO_ROOT roots are;
 *   d_obs[j][m] += o_m;   d_cov[j][a][c] += o_a * o_c for a <= c, and d_cov[j][c][a] receives the same increment.
 * Samples past n_sample or out of range are selected away, never multiplied by zero.  No float atomics.  The order of every sum is a
 * function of (n_sample, n_bin, n_obs, n_root, n_group, FDG_ROOT_SCRATCH_MB) and of the other blocks' own parameters, not of the
 * values of coef.  Every other output of the call carries the bits of the same call without ob (with wg NULL: of the ungrouped
 * call).  Whenever the pass keeps the binned call's segment count (its partials [segment][bin][V], V = n_obs + n_obs (n_obs + 1) / 2,
 * fit in 128 MiB), a row coef[m] = e_k gives d_obs[:, m] the bits of the moments call's d_acc[:, k] and d_cov[:, m, m] those of
 * d_acc2[:, k] (csrc/fdg_binned.hip).
 * These observables combine UNPROJECTED roots: the Matsubara block of this call stays per root.  Sums of PROJECTED roots -- the
 * complex observables of a frequency-resolved measurement -- are the _freq_observables calls below (real coefficients).
 * FDG_E_INVALID: ob NULL, one of its arrays NULL, n_obs == 0, a coefficient that is not finite, d_obs or d_cov the same buffer as the
 * other or as d_acc or d_acc2, one of d_acc and d_acc2 without the other, and the cases of the _grouped calls except those relaxed
 * above; FDG_E_UNSUPPORTED: n_obs > FDG_OBS_MAX and those calls' limits.  All before any device work. */
#define FDG_OBS_MAX 16
typedef struct fdg_observables {
  uint32_t n_obs;      /* 1 .. FDG_OBS_MAX */
  const double *coef;  /* HOST [n_obs][n_root], row-major, finite */
  double *d_obs;       /* device [n_bin][n_obs], added to */
  double *d_cov;       /* device [n_bin][n_obs][n_obs], added to */
} fdg_observables;
int fdg_accumulate_device_observables(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                      int64_t leaf_tile_stride, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                      const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                      uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin,
                                      const fdg_matsubara *mz, const fdg_weight_groups *wg, const fdg_observables *ob, int64_t n_sample,
                                      void *stream);
int fdg_mc_accumulate_device_observables(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                         const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta,
                                         double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight,
                                         const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid,
                                         double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin, const fdg_matsubara *mz,
                                         const fdg_weight_groups *wg, const fdg_observables *ob, int64_t n_sample, void *stream);

/* ---- Frequency observables: linear combinations of the PROJECTED roots, with their covariance -------------------------------------------
 * The reference's measurement multiplies every root's weight by the phase of its own pair of external times and THEN sums the roots
 * into the direct and the exchange component (test/ver4.jl:184-216, `phase(varT, ver4.Tpair[map.ver])` in line 193); a self-energy
 * Sigma(i omega_n) is the sum of its roots, each with its own time pair, over all orders of the series.  The projection above gives a
 * mean and an error bar per (frequency, root); the roots share their samples, so the error of their sum needs the covariance, per
 * frequency, of the real and imaginary parts.  MCIntegration is not part of the reference checkout: no counterpart in the reference;
 * the caller's side of those lines.
 *
 * fdg_[mc_]accumulate_device_freq_observables: the arguments of the _observables calls plus fo, placed after ob.  ob and wg may be
 * NULL.  mz is required: the frequencies, `fermionic`, the time labels, beta and d_T are its own.  In these two calls only, the four
 * per-root arrays of mz may all be NULL (the per-root projected sums are not wanted) or all be given.  coef is a HOST array, row-major
 * [n_obs][n_root], real.  With M = n_obs, for every sample b < n_sample whose bin j is in range, every frequency f and every root k
 * that exists, every step one rounded fp64 operation:
 *   t_k, tau_k, (s, c), tre_k = t_k * c, tim_k = t_k * s exactly as the _matsubara calls form them (t_k = w_g(k) * root_k(b) with wg);
 *   a_m = the left fold of coef[m][k] * tre_k over ascending k, over the roots that exist with coef[m][k] != 0.0; the first product
 *         starts the fold.  b_m = the same fold with tim_k;
 *   z = (a_0 .. a_{M-1}, b_0 .. b_{M-1});   d_fobs[j][f][p] += z_p;   d_fcov[j][f][p][q] += z_p * z_q for p <= q, and
 *         d_fcov[j][f][q][p] receives the same increment.
 * A row without a term leaves its components m and M + m untouched in both arrays, as FDG_NO_ROOT columns are.  The complex
 * observable m at (j, f) is d_fobs[j][f][m] + i d_fobs[j][f][M + m]; d_fcov holds the second moments of the 2 M real components, from
 * which the covariance of the real and imaginary parts of any further real combination follows.
 * No float atomics; samples past n_sample or out of range are selected away, never multiplied by zero; the order of every sum is a
 * function of (n_sample, n_bin, n_freq, n_obs, n_root, n_group, FDG_ROOT_SCRATCH_MB) only, not of the values of coef.  Every other
 * output of the call (d_acc, d_acc2, d_hist, d_hist_bin, the four arrays of mz, ob's arrays) carries the bits of the _observables call
 * without fo (with ob NULL: of the _grouped call): those passes and their plans are not touched (csrc/fdg_binned.hip).
 * FDG_E_INVALID: fo NULL or one of its arrays NULL, n_obs == 0, a coefficient that is not finite, mz NULL, some but not all of mz's
 * four arrays NULL, d_fobs or d_fcov the same buffer as the other or as any other output of the call, and the cases of the
 * _observables calls (ob given) or the _grouped calls with wg optional (ob NULL); FDG_E_UNSUPPORTED: n_obs > FDG_FREQ_OBS_MAX,
 * n_bin * n_freq > FDG_BIN_MAX and those calls' limits.  All before any device work. */
#define FDG_FREQ_OBS_MAX 8
typedef struct fdg_freq_observables {
  uint32_t n_obs;      /* M: 1 .. FDG_FREQ_OBS_MAX */
  const double *coef;  /* HOST [n_obs][n_root], row-major, finite, real */
  double *d_fobs;      /* device [n_bin][n_freq][2 M], added to */
  double *d_fcov;      /* device [n_bin][n_freq][2 M][2 M], added to */
} fdg_freq_observables;
int fdg_accumulate_device_freq_observables(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                           int64_t leaf_tile_stride, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                           const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset,
                                           uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                           double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg,
                                           const fdg_observables *ob, const fdg_freq_observables *fo, int64_t n_sample, void *stream);
int fdg_mc_accumulate_device_freq_observables(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                              const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta,
                                              double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                              const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset,
                                              uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                              double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg,
                                              const fdg_observables *ob, const fdg_freq_observables *fo, int64_t n_sample, void *stream);

/* ---- Adaptive stratified sampling (VEGAS+) ------------------------------------------------------------------------------------------
 * The map above is separable: a ridge along a diagonal (a propagator of k1 + k2, of T[i] - T[j]) is flat in every axis projection, the
 * map stays uniform and the error falls as 1/sqrt(N).  Lepage's VEGAS+ (J. Comput. Phys. 439 (2021) 110386) cuts the unit cube of the
 * map's coordinates into H hypercubes, gives each at least two samples and the rest to the hypercubes where the integrand's standard
 * deviation is largest.  MCIntegration is not part of the reference checkout: no counterpart in the reference.
 *
 * strat[d] >= 1 (a HOST array of n_dim words) is the number of strata of variable d; H = prod strat[d], 1 <= H <= FDG_STRAT_CUBE_MAX;
 * hypercube h has the mixed-radix digits s_d, variable 0 fastest: h = s_0 + strat[0] * (s_1 + strat[1] * (s_2 + ...)).
 * d_start (DEVICE, H + 1 int64) holds the prefix sums of the samples per hypercube in GLOBAL sample indices: start[0] = 0,
 * start[H] = n_total, and n_h = start[h + 1] - start[h] >= 1 (fdg_strat_allocate gives at least 2).  The samples of a hypercube are
 * contiguous, so a sample's hypercube is a function of its index.
 *
 * fdg_vegas_sample_device_strat: for sample b with the global index i = sample_offset + b, every step one rounded fp64 operation,
 *     h   = the hypercube with start[h] <= i < start[h + 1] (a binary search per lane)      -> d_cube[b]  (int32, required)
 *     u   = the uniform of counter (i, d) and key seed, as fdg_vegas_sample_device draws it
 *     v   = ((double)s_d + u) / (double)strat[d];   y = v * G;   c = min((int)y, G - 1)
 *     fr, wd, x, the factor G * wd and the left fold jac_map exactly as in fdg_vegas_sample_device (v may round to 1.0 in the last
 *     stratum: the clamp of c covers it, x is then the last edge)
 *     jac = jac_map * fac_h,   fac_h = (double)n_total / ((double)H * (double)n_h)            -> d_jac[b]
 * With every strat[d] == 1 and start = {0, n_total}, x, d_cell and d_jac carry the bits of fdg_vegas_sample_device ((0 + u) / 1 and
 * * 1.0 are exact).  Counter-based: shards reproduce the unsharded batch.  FDG_E_INVALID: the sampler's cases, strat, d_start or
 * d_cube NULL, strat[d] == 0; FDG_E_UNSUPPORTED: the map's limits, H > FDG_STRAT_CUBE_MAX.  All before any device work.
 *
 * fdg_[mc_]accumulate_device_strat: the arguments of the _vegas calls plus strat, d_cube (the sampler's, int32 [n_sample]) and the
 * per-hypercube moments d_cube_sum, d_cube_sum2 (DEVICE, [H][n_root + 1] doubles each, added to).
 *   d_acc, d_acc2: bit for bit those of the _vegas / moments calls (the same unchanged pass and plan).
 *   d_hist: the training histogram with the cell of (sample, variable) recomputed by the STRATIFIED formula above from the digit of
 *     d_cube[b] and the counter; a sample whose d_cube lies outside [0, H) is selected away from it.  With every strat[d] == 1 and an
 *     all-zero d_cube it carries the bits of fdg_accumulate_device_vegas.
 *   d_cube_sum[h][k] += t_k, d_cube_sum2[h][k] += t_k * t_k with t_k = w_b * root_k(b) (k < n_root; d_weight NULL: t_k = root_k), and
 *     column n_root takes t = w_b * s and t * t, s the coef combination formed exactly as for d_hist.  The column of a root that does
 *     not exist (FDG_NO_ROOT) is left untouched, and so is column n_root when no root exists.
 * d_cube must be non-decreasing over its in-range values (the sampler's is).  Samples with d_cube outside [0, H) and lanes past n_sample
 * enter no per-hypercube sum: selected away, never multiplied by zero.  No float atomics; the sums are bitwise repeatable, and their
 * order is a function of (n_sample, n_root, FDG_ROOT_SCRATCH_MB) only (csrc/fdg_binned.hip).
 * FDG_E_INVALID: the _vegas calls' cases, strat, d_cube, d_cube_sum or d_cube_sum2 NULL, the two the same buffer or one of them the
 * same as d_acc, d_acc2 or d_hist, strat[d] == 0; FDG_E_UNSUPPORTED: H > FDG_STRAT_CUBE_MAX, H * (n_root + 1) > 1 << 24.
 *
 * fdg_strat_allocate (host only): the next iteration's allocation from the per-hypercube moments of column col (leading dimension
 * ld, i.e. cube_sum[h * ld + col]), in fp64, in this order, with n_h and fac_h those of start_old (its own total start_old[H]):
 *  1. var_h = max(0, (sum2_h - sum_h * sum_h / n_h) / (n_h - 1)) / (fac_h * fac_h)
 *  2. d_h = pow(var_h, beta / 2), and 0 for var_h == 0
 *  3. S = the left fold of d_h.  S <= 0, S not finite, beta == 0 or start_old == NULL ("no history"; the moments are then not
 *     read): the allocation is uniform, n_h = 2 + (n_total - 2 H) div H in integers.
 *  4. otherwise n_h = 2 + floor((double)(n_total - 2 H) * (d_h / S)).  The samples left over go one each to h = 0, 1, ... ascending
 *     (wrapping) until the sum is exactly n_total; should rounding have handed out too many, they are taken back one each from
 *     h = H - 1, H - 2, ... among the hypercubes that hold more than 2.
 *  5. start_new[0] = 0, start_new[h + 1] = start_new[h] + n_h.
 * FDG_E_INVALID: a NULL array (start_old may be NULL), H == 0, n_total < 2 H, beta outside [0, 1], col >= ld, a non-finite moment in column col, an old count
 * below 2; FDG_E_UNSUPPORTED: H > FDG_STRAT_CUBE_MAX.  On error start_new is untouched. */
#define FDG_STRAT_CUBE_MAX (1u << 20)
int fdg_vegas_sample_device_strat(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const uint32_t *strat,
                                  const int64_t *d_start, uint64_t seed, uint64_t sample_offset, double *d_x, int64_t x_sample_stride,
                                  int64_t x_col_stride, double *d_jac, int32_t *d_cube, int32_t *d_cell, int64_t n_sample, void *stream);
int fdg_accumulate_device_strat(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                int64_t leaf_tile_stride, const double *d_weight, const double *coef, uint64_t seed,
                                uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                const uint32_t *strat, const int32_t *d_cube, double *d_cube_sum, double *d_cube_sum2, int64_t n_sample,
                                void *stream);
int fdg_mc_accumulate_device_strat(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride, const double *d_T,
                                   int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta, double lambda,
                                   const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                   uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, const uint32_t *strat,
                                   const int32_t *d_cube, double *d_cube_sum, double *d_cube_sum2, int64_t n_sample, void *stream);
int fdg_strat_allocate(const double *cube_sum, const double *cube_sum2, uint32_t ld, uint32_t col, const int64_t *start_old, uint32_t H,
                       int64_t n_total, double beta, int64_t *start_new);

/* ---- Stratified sampling for spherical momenta and weight groups ------------------------------------------------------------------
 * The two halves of the Monte-Carlo step together: loop momenta in a ball (fdg_vegas_sample_device_polar) and several orders per run
 * (the weight groups) under the hypercubes above.  The discrete variable, the projection and the observables stay outside these
 * calls.  MCIntegration is not part of the reference checkout: no counterpart in the reference.
 *
 * fdg_vegas_sample_device_strat_grouped: the arguments of fdg_vegas_sample_device_grouped without the discrete variable, plus strat,
 * d_start and d_cube as fdg_vegas_sample_device_strat takes them.  For sample b with the global index i = sample_offset + b, every
 * step one rounded fp64 operation, in this order,
 *   1. the hypercube h (-> d_cube[b]) and its digits s_d exactly as in fdg_vegas_sample_device_strat;
 *   2. every variable d < n_dim: u the uniform of counter (i, d);  v = ((double)s_d + u) / (double)strat[d];  y = v * G;
 *      c = min((int)y, G - 1);  fr, wd, the value lo + fr * wd and the factor G * wd as everywhere; a polar group's variables are
 *      stratified in (k, theta, phi), the coordinates of the map;
 *   3. the variables of a polar group come out as Cartesian columns by the very statements of fdg_vegas_sample_device_polar;
 *   4. j_g by steps 1-2 of fdg_vegas_sample_device_grouped (the fold over the mask's variables, then its polar groups' factors);
 *   5. j_g * fac_h -> d_jac[g * jac_group_stride + b],  fac_h = (double)n_total / ((double)H * (double)n_h).
 * EVERY group takes fac_h, also a group whose mask leaves variables out: the samples are drawn with the density
 * prod_d (1 / (G wd_d)) / fac_h over all n_dim variables, and an integrand that does not depend on a variable sees that variable's
 * marginal, whose factors cancel between the strata only together with fac_h (stratifying over a variable an integrand does not
 * depend on leaves its estimate unbiased; dropping fac_h for such a group would not).
 * var_mask == NULL with n_group == 0: one jacobian, the full fold (fdg_vegas_sample_device_polar's) times fac_h -> d_jac[b].
 * Identities: with n_polar == 0 and no groups, d_x, d_jac, d_cube and d_cell carry the bits of fdg_vegas_sample_device_strat; with
 * every strat[d] == 1 and start = {0, n_total}, d_x, d_jac and d_cell carry the bits of fdg_vegas_sample_device_grouped (of _polar
 * without groups) with d_cdf == NULL ((0 + u) / 1 and * 1.0 are exact).  Counter-based: shards reproduce the unsharded batch.
 * FDG_E_INVALID / FDG_E_UNSUPPORTED: the cases of fdg_vegas_sample_device_grouped (var_mask NULL with n_group > 0 among them), then
 * those of fdg_vegas_sample_device_strat.  All before any device work.
 *
 * fdg_[mc_]accumulate_device_strat_grouped: the arguments of the _strat calls plus wg.  With g(k) = root_group[k]:
 *   d_acc, d_acc2: bit for bit those of the _grouped calls (the same unchanged moments pass and plan).
 *   d_hist: the grouped training rule (q_g = (w_g s_g)^2, a variable's fold over its owning groups, ascending g) with the cell
 *     recomputed by the stratified formula from d_cube; a sample whose d_cube lies outside [0, H) is selected away.
 *   d_cube_sum, d_cube_sum2 (DEVICE, [H][n_root + n_group] doubles each, added to): column k < n_root takes t_k = w_g(k) * root_k and
 *     t_k * t_k; column n_root + g takes t_g = w_g * s_g and t_g * t_g, s_g the left fold of c_k * r_k over the group's existing
 *     roots, ascending.  Untouched: the column of an FDG_NO_ROOT root and the column of a group with no root that exists.
 * With n_group == 1, root_group all zero and a full mask every output carries the bits of the _strat call, d_cube_sum
 * [H][n_root + 1] included.  No float atomics; samples are selected away, never multiplied by zero; bitwise repeatable; the order of
 * every sum is a function of (n_sample, n_root, n_group, FDG_ROOT_SCRATCH_MB) only.
 * FDG_E_INVALID / FDG_E_UNSUPPORTED: the cases of the _strat calls and of the _grouped calls; H * (n_root + n_group) > 1 << 24 is
 * FDG_E_UNSUPPORTED.  All before any device work.
 *
 * fdg_strat_allocate_cols (host only): fdg_strat_allocate from several columns.  Step 1 gives var_h = the left fold, over cols in the
 * order given, of each column's own var_h, each formed exactly as there; steps 2-5 are unchanged.  n_col == 1 gives the bits of
 * fdg_strat_allocate, which is this call with one column.  FDG_E_INVALID: cols NULL, n_col == 0, a cols[i] >= ld (with start_old),
 * and that call's cases.  On error start_new is untouched. */
int fdg_vegas_sample_device_strat_grouped(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col,
                                          const fdg_vegas_polar *polar, uint32_t n_polar, const uint64_t *var_mask, uint32_t n_group,
                                          int64_t jac_group_stride, const uint32_t *strat, const int64_t *d_start, uint64_t seed,
                                          uint64_t sample_offset, double *d_x, int64_t x_sample_stride, int64_t x_col_stride, double *d_jac,
                                          int32_t *d_cube, int32_t *d_cell, int64_t n_sample, void *stream);
int fdg_accumulate_device_strat_grouped(fdg_graph *g, const double *d_leaf, int64_t leaf_sample_stride, int64_t leaf_leaf_stride,
                                        int64_t leaf_tile_stride, const double *d_weight, const double *coef, uint64_t seed,
                                        uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2,
                                        double *d_hist, const uint32_t *strat, const int32_t *d_cube, double *d_cube_sum,
                                        double *d_cube_sum2, const fdg_weight_groups *wg, int64_t n_sample, void *stream);
int fdg_mc_accumulate_device_strat_grouped(fdg_graph *g, const double *d_K, int64_t k_sample_stride, int64_t k_comp_stride,
                                           const double *d_T, int64_t t_sample_stride, int64_t t_comp_stride, double kF, double beta,
                                           double lambda, const double *d_weight, const double *coef, uint64_t seed,
                                           uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2,
                                           double *d_hist, const uint32_t *strat, const int32_t *d_cube, double *d_cube_sum,
                                           double *d_cube_sum2, const fdg_weight_groups *wg, int64_t n_sample, void *stream);
int fdg_strat_allocate_cols(const double *cube_sum, const double *cube_sum2, uint32_t ld, const uint32_t *cols, uint32_t n_col,
                            const int64_t *start_old, uint32_t H, int64_t n_total, double beta, int64_t *start_new);

/* ---- Markov-chain sampling on the VEGAS map ----------------------------------------------------------------------------------------------
 * The reference's callers of this path sample with a Markov chain: test/hubbard.jl:85 calls integrate(...; solver=:mcmc), and the
 * `measure` of test/ver4.jl:77-92,236-237 and example/strong_coupling_expansion adds weight / abs(weight) / reweight, the estimator of a
 * chain whose stationary density is |integrand|.  A diagram's weight is not separable (propagators tie loop momenta and times together),
 * so a separable map cannot follow it; a chain can.  This is the scheme of MCIntegration's :vegasmc: a Metropolis chain whose proposals
 * are fresh draws through the VEGAS map for a subset of the variables.  MCIntegration is not part of the reference checkout: no
 * counterpart in the reference; the caller's side of test/hubbard.jl:85.
 *
 * One walker per lane, n_walker independent chains, every step one batched evaluation of the proposals.  The walkers are independent,
 * so the error bar comes from the spread across walkers (fdg_chain_reduce_device); no autocorrelation analysis is needed.
 *
 * The walker quantities, every operation one rounded fp64 operation (the library builds with -ffp-contract=off):
 *     x      the point, all n_col columns
 *     fac_d  = G * wd_d, the per-variable jacobian factor of its current value (fdg_vegas_sample_device's factor)
 *     jac    = (..(fac_0 * fac_1) * ..), the left fold over d, as fdg_vegas_sample_device forms it
 *     r_k    the roots at x
 *     s      = (c_k0 * r_k0) + (c_k1 * r_k1) + ...  over the roots that exist, ascending k, left fold; the factor only when coef != NULL
 *              (the training pass's s; 0.0 when no root exists)
 *     t      = jac * s,   a = |t|
 * The stationary density in physical coordinates is p(x) = |s(x)| + gamma q(x), where q = 1 / jac is the map's own normalised density
 * and gamma > 0 an argument.  The gamma q term keeps the chain ergodic wherever the map has support, and its integral is known to be 1,
 * which normalises the result with no reference diagram:
 *     I_k = < r_k / p > / < q / p > = sum (jac * r_k) * d / sum d,     d = 1 / (a + gamma)
 * A move redraws the variables of a mask S through the map and keeps the others.  The Metropolis ratio is (a' + gamma) / (a + gamma)
 * for every mask: the factors of the unchanged variables cancel, the redrawn ones cancel against the proposal density.
 * The accept rule is   u * (a + gamma) < (a' + gamma),   each side one rounded operation, with u = what fdg_fill_uniform_device writes
 * for counter (sample_offset + b, FDG_VEGAS_DIM_MAX) and the step's key: a variable index that no sampler uses.
 * A proposal at which any existing root is non-finite, or whose t' is non-finite, counts as f = 0 there: its roots are taken as 0.0
 * and a' = 0.  The value is selected, never multiplied, so an inf or nan poisons nothing; the normal rule applies to it.
 * Roots that do not exist (FDG_NO_ROOT) are skipped in s, and their columns of the state and of the sums are never written.  Lanes
 * past n_walker write nothing.
 *
 * fdg_chain_propose_device: d_x, d_xp are component-major (sample stride 1) with column strides x_col_stride, xp_col_stride
 * (>= n_walker), n_col columns each; d_fac, d_facp are [n_dim][n_walker].  For walker b:
 *     variable d in mask:      xp[col[d]][b] and facp[d][b] are what fdg_vegas_sample_device computes for counter (sample_offset + b, d)
 *                              and key seed: x the same bits, fac = G * wd_d
 *     variable d not in mask:  xp[col[d]][b] = x[col[d]][b], facp[d][b] = fac[d][b]
 *     a column col does not name: copied from d_x
 * so d_xp is a complete input of the evaluator.  d_grid is the map on the device, read where the sampler reads it; col a HOST array
 * (NULL: col[d] = d).  FDG_E_INVALID: a NULL array, d_x == d_xp or d_fac == d_facp, a col[d] >= n_col, a column stride < n_walker, mask
 * with a bit at or above n_dim, n_dim or n_grid 0; FDG_E_UNSUPPORTED: the map's limits exceeded.  n_dim = 64 is allowed.
 *
 * fdg_chain_step_device (leaf form: the n_col = n_leaf columns of d_xp are the graph's leaves, as in fdg_accumulate_device_strat's leaf
 * form) and fdg_mc_chain_step_device (Monte-Carlo form: d_xp is one [n_loop * dim + n_tau][n_walker] array, momentum components first
 * and then the times; kF, beta, lambda as in fdg_mc_eval_device): the roots of the proposals are evaluated chunk by chunk into the
 * handle's root scratch by the route fdg_eval_device / fdg_mc_eval_device takes (the same root bits on every back end and layout), then
 * one kernel does, per walker: the fold s', t', a'; the accept rule (FDG_CHAIN_INIT: accepted unconditionally, no u is drawn: the first
 * placement of the walkers); the selection of x, fac, root, a from the proposal, or they are kept; and
 *     FDG_CHAIN_MEASURE:  sum[k][b] += (jac * r_k) * d  for k < R,  sum[R][b] += d     on the state AFTER the selection (the product is
 *                         rounded before the addition);
 *     n_accept[b] += 1 on acceptance (int32; d_n_accept may be NULL).
 * The state is caller-owned device memory: x [n_col][n_walker] (column stride x_col_stride), fac [n_dim][n_walker], root
 * [n_root][n_walker], a [n_walker], sum [n_root + 1][n_walker] (may be NULL without FDG_CHAIN_MEASURE).  coef is a HOST array of n_root
 * finite factors or NULL.  The result is a function of the arguments only: every word is written by one lane, a walker's sums are
 * added in step order, and nothing depends on FDG_ROOT_SCRATCH_MB, the launch shape or how the walkers are sharded (a shard passes the
 * start of its range as part of sample_offset).  FDG_E_INVALID: a NULL handle or array, any two of the state, proposal and sum arrays
 * the same buffer, gamma not finite or <= 0, a coef that is not finite, unknown flags, n_dim 0, n_col that does not match the graph's
 * leaves (leaf form) or the tables' n_loop * dim + n_tau (Monte-Carlo form), a column stride < n_walker, n_walker < 0; the Monte-Carlo
 * form before fdg_graph_specialize_fused; FDG_E_UNSUPPORTED: n_dim > FDG_VEGAS_DIM_MAX.  All before any device work.
 *
 * fdg_chain_reduce_device: from d_sum [n_root + 1][n_walker], with A_c(b) = sum[c][b] and R = n_root, adds into d_out (3 R + 2 doubles)
 *     d_out[c]             += S_c = sum_b A_c(b)            c = 0 .. R
 *     d_out[R + 1 + c]     += Q_c = sum_b A_c(b)^2          c = 0 .. R
 *     d_out[2 R + 2 + k]   += X_k = sum_b A_k(b) * A_R(b)   k = 0 .. R - 1
 * No float atomics; bitwise reproducible; the order of every sum is a function of (n_walker, n_root) only: one workgroup per output,
 * lane t of 256 adds the terms b = t, t + 256, .. in ascending b, the 256 partials are added pairwise (stride 128, 64, .., 1).  Every
 * column of d_sum is read, also a root's that does not exist (the caller zeroes d_sum before the first measured step). */
#define FDG_CHAIN_INIT 1u
#define FDG_CHAIN_MEASURE 2u
int fdg_chain_propose_device(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask,
                             uint64_t seed, uint64_t sample_offset, const double *d_x, int64_t x_col_stride, const double *d_fac,
                             double *d_xp, int64_t xp_col_stride, double *d_facp, int64_t n_walker, void *stream);
int fdg_chain_step_device(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col, uint32_t n_dim,
                          const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags, double *d_x,
                          int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept,
                          int64_t n_walker, void *stream);
int fdg_mc_chain_step_device(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                             const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma, uint64_t seed,
                             uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac, double *d_root,
                             double *d_a, double *d_sum, int32_t *d_n_accept, int64_t n_walker, void *stream);
int fdg_chain_reduce_device(const double *d_sum, uint32_t n_root, int64_t n_walker, double *d_out, void *stream);

/* ---- Markov chain with a Matsubara-projected weight and measurement ----------------------------------------------------------------------
 * The integrand of the chain's own target, Sigma(i omega_n) of test/hubbard.jl, is complex:
 *     w = sum_k c_k r_k e^{i omega (T[out_k] - T[in_k])}
 * The chain walks on |w| at ONE frequency (weight_freq) and measures every root at every frequency of the descriptor.  The phase has to
 * be part of the weight: a chain on the unprojected |s| with the phases multiplied in afterwards is another, worse estimator, and none
 * at all where the unprojected sum cancels.  MCIntegration is not part of the reference checkout: no counterpart in the reference; the
 * caller's side of test/hubbard.jl:85 with the measure of test/ver4.jl:193.
 *
 * fdg_chain_propose_device and fdg_chain_reduce_device serve as they are, and the state (x, fac, root, a) keeps its layout; only d_sum
 * grows.  Per walker, every line one rounded fp64 operation (no FMA), in this order:
 *
 * The phase of root k at frequency f for a point p (the proposal xp, or the state x):
 *     tau = p[root_col_out[k]] - p[root_col_in[k]];   x = tau / beta
 *     (s, c) = the phase of fdg_matsubara_phase from x on, with the multiplier of (freq[f], fermionic)      (csrc/fdg_matsubara.h)
 * The weight of a proposal, over the roots j that exist in ascending order, (s_j, c_j) at weight_freq from the proposal's own times:
 *     term = coef ? coef_j * r_j : r_j;   pr = term * c_j;   pi = term * s_j
 *     re = re + pr;   im = im + pi                   (left folds; the first term is assigned, not added to 0; no root: 0.0)
 *     tre = jac' * re;   tim = jac' * im
 *     q   = tre * tre + tim * tim;   a' = sqrt(q)    (the two squares, their sum and the root each rounded once; fp64 sqrt is
 *                                                     correctly rounded on host and device)
 * A proposal at which an existing root, tre, tim or q is not finite counts as f = 0: its roots are taken as 0.0 and a' = 0, selected
 * and never multiplied.  (q is in the list because a finite tre or tim above 1.3e154 squares to inf: a walker with a = inf would be
 * accepted and never leave.  The plain step's a = |t| has no such range.)
 * The accept rule, FDG_CHAIN_INIT, n_accept and the selection of x, fac, root, a are the plain step's, on the same Philox counter.
 * FDG_CHAIN_MEASURE, on the state AFTER the selection, with R = n_root and F = n_freq:
 *     d = 1 / (a + gamma)
 *     for every root k that exists:   w = (jac * r_k) * d;   for every f, (s, c) from the state's times:
 *         sum[2 (f R + k)][b]     += w * c
 *         sum[2 (f R + k) + 1][b] += w * s
 *     sum[2 F R][b] += d
 * d_sum is [2 F R + 1][n_walker]; fdg_chain_reduce_device(d_sum, 2 F R, ..) reduces it, one ratio per (frequency, root, component).
 * The columns of a root that does not exist are never written, in root and in sum; its time columns are not read and may be anything.
 * The times are columns of x that the map draws or the caller fixes: they are taken as finite.  With fermionic = 0 and freq = {0} the
 * phase is exactly (0, 1) and the state is the plain step's bit for bit (wherever tre * tre neither overflows nor underflows: 1e-154 < |tre| < 1.3e154).
 *
 * The Metropolis ratio stays (a' + gamma) / (a + gamma): the stationary density is |w(x)| + gamma q(x) with the same q, and the
 * argument of the plain step needs of the weight only that it is a non-negative function of the point.
 *
 * The result is a function of the arguments only, as for the plain step (FDG_ROOT_SCRATCH_MB, launch shape, shards).
 * FDG_E_INVALID: everything the plain step refuses; a NULL descriptor, freq, root_col_in or root_col_out; n_freq == 0;
 * weight_freq >= n_freq; beta not finite or <= 0; a time column >= n_col of a root that exists.  FDG_E_UNSUPPORTED: the plain step's
 * case, n_freq > FDG_MATSUBARA_FREQ_MAX.  All before any device work. */
typedef struct fdg_chain_matsubara {
  uint32_t n_freq;              /* 1 .. FDG_MATSUBARA_FREQ_MAX */
  int32_t fermionic;            /* != 0: omega_n = (2n+1) pi / beta;  0: 2n pi / beta */
  const int32_t *freq;          /* HOST [n_freq]: the n of every frequency */
  uint32_t weight_freq;         /* index into freq: the frequency whose projected sum is the chain's weight */
  const uint32_t *root_col_in;  /* HOST [n_root]: 0-based column of x / xp that holds t_in of root k */
  const uint32_t *root_col_out; /* HOST [n_root] */
  double beta;                  /* > 0 */
} fdg_chain_matsubara;
int fdg_chain_step_device_matsubara(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col,
                                    uint32_t n_dim, const double *coef, double gamma, uint64_t seed, uint64_t sample_offset,
                                    unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac, double *d_root, double *d_a,
                                    double *d_sum, int32_t *d_n_accept, const fdg_chain_matsubara *mz, int64_t n_walker, void *stream);
int fdg_mc_chain_step_device_matsubara(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                                       const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma,
                                       uint64_t seed, uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride,
                                       double *d_fac, double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept,
                                       const fdg_chain_matsubara *mz, int64_t n_walker, void *stream);

/* ---- Markov chain with weight groups and reweighting between orders ---------------------------------------------------------------------
 * A diagram series integrated with all its orders at once gives every order its own variables (MCIntegration's dof; "Weight groups"
 * above).  This is MCIntegration's :vegasmc with several integrands: group g has the variables of var_mask[g], jac_g is the jacobian of
 * those variables only, s_g the coef combination of the group's roots and rho_g > 0 a reweight factor that balances the orders.  The
 * stationary density in physical coordinates is
 *     p(x) = sum_g rho_g |s_g(x)| q_notg(x) + gamma q(x),     q_notg = prod_{d not in g} 1 / fac_d
 * (the map's density of the variables the group does not integrate), in the map's coordinates pi(y) = a(y) + gamma with
 * a = sum_g rho_g |jac_g s_g|.  The Metropolis ratio stays (a' + gamma) / (a + gamma) for every move mask: the argument of the plain
 * step needs of a only that it is a non-negative function of the point.  The estimate is
 *     I_k = sum (jac_g(k) * r_k) * d / sum d,     d = 1 / (a + gamma)
 * since the variables outside the group integrate to 1 under q.  MCIntegration is not part of the reference checkout: no counterpart
 * in the reference; the caller's side of test/hubbard.jl:81-85 with more than one order.
 *
 * fdg_chain_propose_device and fdg_chain_reduce_device serve as they are; the state (x, fac, root, a) and d_sum keep the layout of the
 * plain step (mz == NULL) or of the projected step (mz != NULL).  Per walker, every line one rounded fp64 operation (no FMA), the first
 * term of every fold assigned, not added to 0, in this order:
 *     jac_g = the left fold of fac_d over ascending d with bit d in var_mask[g]; an empty mask gives 1.0
 *   mz == NULL:
 *     s_g = (c_k0 * r_k0) + (c_k1 * r_k1) + ...  over the group's roots that exist, ascending k; the factor only with coef != NULL
 *     t_g = jac_g * s_g;   a_g = |t_g|
 *   mz != NULL, (s_k, c_k) the phase of root k at weight_freq from the proposal's own times, as in the projected step:
 *     term = coef ? coef_k * r_k : r_k;   re_g = re_g + term * c_k;   im_g = im_g + term * s_k      (left folds over the group's roots)
 *     tre_g = jac_g * re_g;   tim_g = jac_g * im_g;   q_g = tre_g * tre_g + tim_g * tim_g;   a_g = sqrt(q_g)
 *   a' = the left fold of rho_g * a_g over ascending g among the groups that have a root that exists (reweight == NULL: of a_g, no
 *        product is formed); no root at all: 0.0.  A group without such a root takes no part anywhere.
 * A proposal at which an existing root, any t_g (any tre_g, tim_g or q_g) or a' is not finite counts as f = 0: all its roots are taken
 * as 0.0 and a' = 0, selected and never multiplied.
 * The accept rule, FDG_CHAIN_INIT, n_accept and the selection of x, fac, root, a are the plain step's, on the same Philox counter.
 * FDG_CHAIN_MEASURE, on the state AFTER the selection, jac_g from the state's fac:
 *     d = 1 / (a + gamma)
 *   mz == NULL:  sum[k][b] += (jac_g(k) * r_k) * d  for every root k that exists,  sum[R][b] += d
 *   mz != NULL:  w = (jac_g(k) * r_k) * d;  sum[2 (f R + k)][b] += w * c,  sum[2 (f R + k) + 1][b] += w * s  for every f, the phases
 *                from the state's times;  sum[2 F R][b] += d
 * The columns of a root that does not exist are never written.  A variable of no group moves and is copied like any other and enters
 * no jacobian.
 *
 * With n_group == 1, a mask of all n_dim variables and reweight == NULL the state and the sums are bit for bit those of
 * fdg_[mc_]chain_step_device (mz == NULL) or of fdg_[mc_]chain_step_device_matsubara (mz != NULL).
 * The result is a function of the arguments only, as for the plain step (FDG_ROOT_SCRATCH_MB, launch shape, shards).
 * FDG_E_INVALID: everything the plain step refuses and, with mz != NULL, everything the projected step refuses of its descriptor; a
 * NULL cg, root_group or var_mask; n_group == 0; root_group[k] >= n_group for a root that exists; a mask bit at or above n_dim; a
 * reweight that is not finite or <= 0.  FDG_E_UNSUPPORTED: those calls' cases, n_group > FDG_WEIGHT_GROUP_MAX.  All before any device
 * work. */
typedef struct fdg_chain_groups {
  uint32_t n_group;             /* 1 .. FDG_WEIGHT_GROUP_MAX */
  const uint32_t *root_group;   /* HOST [n_root]: the group of root k (ignored for FDG_NO_ROOT roots) */
  const uint64_t *var_mask;     /* HOST [n_group]: bit d set = variable d belongs to the group; an empty mask is allowed */
  const double *reweight;       /* HOST [n_group], finite and > 0, or NULL: no factor is applied */
} fdg_chain_groups;
int fdg_chain_step_device_grouped(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col,
                                  uint32_t n_dim, const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags,
                                  double *d_x, int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum,
                                  int32_t *d_n_accept, const fdg_chain_matsubara *mz, const fdg_chain_groups *cg, int64_t n_walker,
                                  void *stream);
int fdg_mc_chain_step_device_grouped(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                                     const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma, uint64_t seed,
                                     uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac,
                                     double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept, const fdg_chain_matsubara *mz,
                                     const fdg_chain_groups *cg, int64_t n_walker, void *stream);

/* ---- Markov chain with a discrete external variable and per-bin measurement ---------------------------------------------------------------
 * The vertex-function caller of this path samples over (K, T, ExtKidx) with ExtKidx = MCIntegration.Discrete(1, Nk), and its `measure`
 * adds weight / |weight| * factor into observable[extKidx, :] (test/ver4.jl:77-92, 224-237; example/strong_coupling_expansion does the
 * same).  One chain run then yields the roots on a grid of external momenta, every grid point with its own error bar.  MCIntegration
 * is not part of the reference checkout: no counterpart in the reference; the caller's side of test/ver4.jl.
 *
 * The discrete variable is one more coordinate of the map, the one of "A discrete external variable" above: in the map's coordinates
 * a uniform u, its value j = the number of interior edges cdf[1 .. n_bin - 1] that are <= u (fdg_vegas_sample_device_discrete's rule),
 * p_j = cdf[j + 1] - cdf[j], and its jacobian factor fd = 1.0 / p_j, one rounded division.  It is shared by every weight group, as in
 * the direct sampler's binned calls.  The state grows by it:
 *     d_fac, d_facp   [n_dim + 1][n_walker]; row n_dim holds fd
 *     d_bin, d_binp   int32 [n_walker]: the 0-based j of the state and of the proposal
 * x, root and a keep their layout.
 *
 * fdg_chain_propose_device_discrete: fdg_chain_propose_device's arguments and results (the continuous variables and the copied
 * columns, the same bits), and then
 *     move_discrete != 0:  u = what fdg_fill_uniform_device writes for counter (sample_offset + b, n_dim), the direct sampler's counter;
 *                          binp[b] = j', facp[n_dim][b] = 1.0 / p_j', xp[ext_col[e]][b] = ext[j'][e] for e < n_ext
 *     move_discrete == 0:  binp[b] = bin[b], facp[n_dim][b] = fac[n_dim][b]; the ext_col columns are copied from d_x like any column
 *                          col does not name
 * d_cdf [n_bin + 1] and d_ext [n_bin][n_ext] lie on the device, ext_col is a HOST array of n_ext columns.  FDG_E_INVALID: everything
 * fdg_chain_propose_device refuses; a NULL d_cdf, d_bin or d_binp; d_bin == d_binp; n_bin 0; n_ext > 0 without d_ext or ext_col; an
 * ext_col that repeats, names a column of col or one >= n_col.  FDG_E_UNSUPPORTED: that call's cases; n_dim == FDG_VEGAS_DIM_MAX (that
 * counter belongs to the accept rule); n_bin > FDG_CHAIN_BIN_MAX; n_ext > FDG_VEGAS_EXT_MAX.  All before any device work.
 *
 * fdg_chain_step_device_binned and fdg_mc_chain_step_device_binned: the grouped entries' arguments plus n_bin, d_binp, d_bin.  mz and
 * cg may each be NULL; a NULL cg is one group holding every root that exists and every variable, without a factor, as the plain
 * entries build it.  Per walker the statements are the grouped step's, in its order, with
 *     jac_g = the left fold of fac_d over the group's mask (an empty mask: 1.0), then one more rounded product jac_g * fd, applied
 *             last; for every group, in the weight of the proposal (facp) and in the measurement (the state's fac)
 * The weight a, the poison rules (an overflowing fd * jac_g s_g poisons like any non-finite t_g), the accept rule
 * u * (a + gamma) < (a' + gamma) on counter (sample_offset + b, FDG_VEGAS_DIM_MAX), FDG_CHAIN_INIT and n_accept are unchanged.  The
 * Metropolis ratio stays (a' + gamma) / (a + gamma): a is still a non-negative function of the point in the map's coordinates, and the
 * proposal of the discrete coordinate is uniform both ways.  On acceptance bin[b] = binp[b] and the rows 0 .. n_dim of fac are copied.
 * FDG_CHAIN_MEASURE, on the state AFTER the selection, with j = bin[b], R = n_root, F = n_freq, d = 1 / (a + gamma):
 *     mz == NULL:  d_sum is [n_bin R + 1][n_walker];      sum[j R + k][b] += (jac_g(k) * r_k) * d;   sum[n_bin R][b] += d
 *     mz != NULL:  d_sum is [2 n_bin F R + 1][n_walker];  w = (jac_g(k) * r_k) * d;  sum[2 ((j F + f) R + k)][b] += w * c,  the next
 *                  column += w * s  for every f;  sum[2 n_bin F R][b] += d
 * A walker writes only the columns of its current bin, through a row address of its own: no loop over the bins, nothing multiplied by
 * zero, no atomics; every word belongs to one lane.  The columns of a root that does not exist and of every other bin are never
 * written.  A bin outside [0, n_bin), which fdg_chain_propose_device_discrete never writes, measures nothing in that step.
 * fdg_chain_reduce_device(d_sum, n_bin R [2 n_bin F R], ..) reduces it, and I_{j,k} = S_{j R + k} / S_last is the integral over the
 * continuous variables at configuration j: the weight carries 1 / p_j, as in the direct sampler's binned calls.
 *
 * With n_bin = 1, cdf = {0, 1} and n_ext = 0, fd = 1.0 and x, fac rows 0 .. n_dim - 1, root, a, sum and n_accept are bit for bit those
 * of fdg_[mc_]chain_step_device, .._matsubara or .._grouped with the same descriptors.
 * The result is a function of the arguments only, as for the plain step (FDG_ROOT_SCRATCH_MB, launch shape, shards).
 * FDG_E_INVALID: everything the plain step refuses and, of a descriptor that is given, everything the projected and the grouped step
 * refuse; n_bin 0; a NULL d_bin or d_binp; d_bin == d_binp, or either the same buffer as another array.  FDG_E_UNSUPPORTED: those
 * calls' cases, n_bin > FDG_CHAIN_BIN_MAX.  All before any device work. */
#define FDG_CHAIN_BIN_MAX 64
int fdg_chain_propose_device_discrete(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col,
                                      uint64_t mask, uint64_t seed, uint64_t sample_offset, const double *d_x, int64_t x_col_stride,
                                      const double *d_fac, double *d_xp, int64_t xp_col_stride, double *d_facp, int move_discrete,
                                      const double *d_cdf, uint32_t n_bin, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                      const int32_t *d_bin, int32_t *d_binp, int64_t n_walker, void *stream);
int fdg_chain_step_device_binned(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col,
                                 uint32_t n_dim, const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags,
                                 double *d_x, int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum,
                                 int32_t *d_n_accept, const fdg_chain_matsubara *mz, const fdg_chain_groups *cg, uint32_t n_bin,
                                 const int32_t *d_binp, int32_t *d_bin, int64_t n_walker, void *stream);
int fdg_mc_chain_step_device_binned(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                                    const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma, uint64_t seed,
                                    uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac,
                                    double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept, const fdg_chain_matsubara *mz,
                                    const fdg_chain_groups *cg, uint32_t n_bin, const int32_t *d_binp, int32_t *d_bin, int64_t n_walker,
                                    void *stream);

/* ---- Markov chain with spherical momentum variables --------------------------------------------------------------------------------------
 * Every caller of the chain in the reference draws its loop momenta as MCIntegration.FermiK, a modulus and a direction over a ball
 * (test/hubbard.jl:85, test/ver4.jl:77-92, 224-237, example/benchmark.jl:46).  This is "Spherical momentum variables" above in the
 * chain's proposal.  MCIntegration is not part of the reference checkout: no counterpart in the reference.
 *
 * Unlike the direct sampler, which folds the polar measure into its one jacobian, the chain keeps the measure's factors PER VARIABLE
 * in the rows of fac that it already carries, each row a function of its own variable alone, so that the step's left fold over a
 * group's mask is the jacobian of the polar measure: no step entry, and nothing of the state's layout, changes.
 *
 * fdg_chain_propose_device_polar: fdg_chain_propose_device_discrete's arguments and results, plus the groups polar[0 .. n_polar) of
 * fdg_vegas_sample_device_polar (HOST array).  d_cdf == NULL: no discrete variable; move_discrete, n_bin, d_ext, n_ext, ext_col, d_bin
 * and d_binp are ignored, d_fac and d_facp have n_dim rows and n_dim = 64 is allowed.  A variable of no group behaves as in
 * fdg_chain_propose_device, the discrete variable as in fdg_chain_propose_device_discrete.  For a group {var, dim, col[]} whose
 * variables the mask names, with k, theta, phi the values drawn through the map for the variables var, var + 1, var + 2 (dim 2:
 * k, phi), each by fdg_vegas_sample_device's statements on counter (sample_offset + b, d) -- the direct sampler's counters -- and
 * f_d = G * wd_d, every line one rounded fp64 operation (no FMA), in this order:
 *     (st, ct) = fdg_sincos(theta);   (sp, cp) = fdg_sincos(phi)
 *   dim 3:  ks = k * st;   xp[col[0]] = ks * cp;   xp[col[1]] = ks * sp;   xp[col[2]] = k * ct
 *           facp[var] = (f_k * k) * k;   facp[var + 1] = f_theta * st;   facp[var + 2] = f_phi
 *   dim 2:  xp[col[0]] = k * cp;   xp[col[1]] = k * sp;   facp[var] = f_k * k;   facp[var + 1] = f_phi
 * so a full proposal's xp is fdg_vegas_sample_device_polar's x bit for bit, and the product of the rows of facp its jac up to the
 * order of the products.  st >= 0 on [0, fl(pi)], so no factor is negative; k = 0 gives the factor 0, hence a' = 0, which is finite
 * and no poison.  A group whose variables the mask does not name is kept: its rows of fac are copied, and its columns with all the
 * columns nobody redraws.  A move redraws a group whole or not at all: the state does not hold (k, theta, phi), which moving the
 * modulus or the direction alone would need.  The col entry of a grouped variable is not read.
 * With n_polar == 0 the results are bit for bit those of fdg_chain_propose_device (d_cdf == NULL) or of
 * fdg_chain_propose_device_discrete.
 * FDG_E_INVALID / FDG_E_UNSUPPORTED, in this order: everything fdg_chain_propose_device refuses; with d_cdf != NULL everything
 * fdg_chain_propose_device_discrete refuses of the discrete variable's arguments; n_polar > FDG_VEGAS_POLAR_MAX (unsupported); a NULL
 * polar with n_polar > 0; a dim that is not 2 or 3, a group that reaches past n_dim, two groups that share a variable; a group's
 * column >= n_col, a column named twice among the col entries of the variables of no group, the groups' columns and ext_col; a mask
 * that names some but not all variables of a group.  All before any device work. */
int fdg_chain_propose_device_polar(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask,
                                   uint64_t seed, uint64_t sample_offset, const double *d_x, int64_t x_col_stride, const double *d_fac,
                                   double *d_xp, int64_t xp_col_stride, double *d_facp, int move_discrete, const double *d_cdf,
                                   uint32_t n_bin, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col, const int32_t *d_bin,
                                   int32_t *d_binp, const fdg_vegas_polar *polar, uint32_t n_polar, int64_t n_walker, void *stream);

/* ---- Markov chain with local shift moves in the map's coordinate -----------------------------------------------------------------------
 * The solver that the reference's test/hubbard.jl:85 asks for (integrate(...; solver=:mcmc)) walks by local moves: small displacements
 * of one variable at a time, not independent fresh draws.  Diagram weights depend on differences of times and momenta; a separable map
 * cannot follow such a ridge, and a whole-variable redraw lands off it most of the time.  MCIntegration is not part of the reference
 * checkout: no counterpart in the reference.
 *
 * With x = map(y), the stationary density of the chain in the map's uniform coordinate y is exactly a + gamma, where
 * a = sum_g rho_g |jac_g s_g| is pi / q as before.  So the step's rule u (a + gamma) < a' + gamma is the correct Metropolis rule for ANY
 * proposal that is symmetric in y.  A redraw is the uniform, symmetric proposal in y; the shift y' = y + t h (mod 1), t uniform in
 * [-1, 1), is another one: the density of y' given y depends on (y' - y) mod 1 only, and is even in it.  Weight groups, the Matsubara
 * weight and the per-bin measurement stay valid: a group's density is uniform in the y of the variables it does not own.  No step,
 * select or reduce entry changes; only the proposal does.
 *
 * fdg_chain_propose_device_local: fdg_chain_propose_device_polar's arguments and results, with local_mask and width behind mask.  A
 * variable of local_mask is SHIFTED; a variable of mask is redrawn as before; every other one is copied.  width is a HOST array of
 * [n_dim] entries, the half width h_d of the shift of variable d as a fraction of the map's unit interval, read only where local_mask
 * has a bit; hG_d = width[d] * (double)n_grid is formed on the host.  For a shifted variable d, with e[0 .. G] row d of the grid,
 * xv = x[col[d]] the walker's value and u the uniform of counter (sample_offset + b, d) -- the column a redraw of d would use; a variable
 * is redrawn or shifted in one step, never both -- every line one rounded fp64 operation (no FMA), in this order:
 *   the inverse of the map:
 *     c  = the number of interior edges e[1 .. G - 1] that are <= xv (a binary search per lane; G = 1 searches nothing)
 *     lo = e[c];   wd = e[c + 1] - lo;   fr = (xv - lo) / wd;   fr = 0 when wd == 0 or fr is not >= 0;   fr = 1 when fr > 1
 *     yy = (double)c + fr                                        in cells: 0 <= yy <= G
 *   the shift:
 *     t = (u + u) - 1.0;   y1 = yy + t * hG_d
 *     if y1 < 0: y1 = y1 + G;   if y1 >= G: y1 = y1 - G           one wrap suffices because width <= 0.5
 *     c' = min((uint32_t)(int)y1, G - 1);   fr' = y1 - c'
 *   the map again, the tail of fdg_vegas_sample_device's statements:
 *     xp[col[d]] = lo' + fr' * wd';   facp[d] = G * wd'
 * A shift is meant for a placed walker: after FDG_CHAIN_INIT a value lies inside its row.  A value outside it (or a nan) is clamped
 * to the row's ends by the statements above and not faulted on: every index into the grid lies in [0, G].
 * The discrete variable and the polar groups can only be redrawn.  The state holds Cartesian columns and no (k, theta, phi); inverting
 * that with pinned bits is out of scope here, as are local moves of the discrete variable.
 * With local_mask == 0 the results are bit for bit those of fdg_chain_propose_device_polar (width is not read and may be NULL).
 * FDG_E_INVALID / FDG_E_UNSUPPORTED, in this order: everything fdg_chain_propose_device_polar refuses; a bit of local_mask at or above
 * n_dim (invalid); mask & local_mask != 0 (invalid); local_mask naming a variable of a polar group (unsupported); width == NULL with
 * local_mask != 0 (invalid); a named width[d] that is not finite or not in (0, 0.5] (invalid).  All before any device work. */
int fdg_chain_propose_device_local(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask,
                                   uint64_t local_mask, const double *width, uint64_t seed, uint64_t sample_offset, const double *d_x,
                                   int64_t x_col_stride, const double *d_fac, double *d_xp, int64_t xp_col_stride, double *d_facp,
                                   int move_discrete, const double *d_cdf, uint32_t n_bin, const double *d_ext, uint32_t n_ext,
                                   const uint32_t *ext_col, const int32_t *d_bin, int32_t *d_binp, const fdg_vegas_polar *polar,
                                   uint32_t n_polar, int64_t n_walker, void *stream);

/* ---- Observables of the chain: sums of roots with their covariance -------------------------------------------------------
 * Every caller of the chain in the reference reports a SUM of roots (test/ver4.jl:184-216: a direct and an exchange component;
 * Sigma(i omega_n) of test/hubbard.jl: the sum over all orders).  All roots share their walkers, so the error of a sum is not the
 * quadrature of the roots' errors: it needs the cross moments sum_b A_k(b) A_l(b), which fdg_chain_reduce_device does not form.  An
 * observable is linear in the walkers' sums, so one reduction behind the chain provides them; no step changes.
 *
 * d_sum is any chain's d_sum: [n_columns][n_walker], stride n_walker.  The window is the columns col_base .. col_base + n_use - 1,
 * norm_col the normalisation's column (the last one of every layout), outside the window.  The layouts with bins and frequencies are
 * blocks -- R columns at j R for bin j; 2 R interleaved real / imaginary columns at 2 (j F + f) R for bin j, frequency f -- and an
 * observable lives in one block: one call per block.  coef is a HOST array [n_obs][n_use], copied before the call returns.
 *
 * With M = n_obs and A_c(b) = d_sum[c][b], every line one rounded fp64 operation, no FMA:
 *     O_m(b) = the left fold of coef[m][c] * A_{col_base + c}(b) over ascending c, over the c with coef[m][c] != 0.0; the first product
 *              starts the fold (no 0.0 + in front).                O_M(b) = A_{norm_col}(b)
 *     d_out[p]                 += S_p  = sum_b O_p(b)              p = 0 .. M
 *     d_out[M + 1 + idx(p, q)] += P_pq = sum_b O_p(b) * O_q(b)     p <= q,   idx(p, q) = p (M + 1) - p (p - 1) / 2 + (q - p)
 * V = (M + 1) + (M + 1) (M + 2) / 2 doubles, the upper triangle packed row-major.  A column whose coefficient is zero in every row is
 * never read: a nan there reaches no output (zeros are selected away, never multiplied).  A row without a term leaves its S entry
 * and its row and column of P untouched in d_out.
 * No float atomics; bitwise reproducible; the order of every sum is a function of n_walker alone, not of coef, n_obs or the kernel's
 * instance: with W = min(max(ceil(n_walker / 256), 1), FDG_CHAIN_OBS_GROUPS), lane t of workgroup w adds from +0.0 the terms of the
 * walkers b = 256 w + t + 256 W i, i = 0, 1, .. ascending; the 256 lane partials of a workgroup are added pairwise (stride 128, 64,
 * .., 1); per output, lane t of 256 adds the workgroup partials w = t, t + 256, .. ascending from +0.0, then the same pairwise tree,
 * then d_out[v] = d_out[v] + total (fdg_chain_reduce_device's scheme on [V][W] partials).
 * The partials and the table of the live columns lie in d_work, which the caller provides: fdg_chain_reduce_observables_work_bytes
 * (n_obs, n_use) bytes, 0 for arguments the entry refuses.  The entry takes no graph handle and allocates nothing.
 * In this order, all before any device work.  FDG_E_INVALID: NULL d_sum, d_out or d_work; NULL coef; two of d_sum, d_out and d_work the
 * same buffer; n_walker < 0; n_obs == 0; n_use == 0.  FDG_E_UNSUPPORTED: n_obs > FDG_CHAIN_OBS_MAX; n_use > FDG_CHAIN_OBS_COL_MAX.
 * FDG_E_INVALID: a coefficient that is not finite; norm_col inside the window.  n_walker == 0 returns FDG_OK and writes nothing. */
#define FDG_CHAIN_OBS_MAX 16       /* rows per call */
#define FDG_CHAIN_OBS_COL_MAX 1024 /* columns of the window */
#define FDG_CHAIN_OBS_GROUPS 1024  /* workgroups of the first stage */
size_t fdg_chain_reduce_observables_work_bytes(uint32_t n_obs, uint32_t n_use);
int fdg_chain_reduce_device_observables(const double *d_sum, int64_t n_walker, uint32_t col_base, uint32_t n_use, uint32_t norm_col,
                                        const double *coef, uint32_t n_obs, double *d_out, void *d_work, void *stream);

/* Device workspace control: the interpreter keeps per-sample overflow slots in
 * an HBM panel owned by the handle; it is sized on first use for the number of
 * resident waves.  This releases it (and any loaded module). */
int fdg_graph_release_device(fdg_graph *g);

/* ---- multi-GPU -------------------------------------------------
 * Samples are sharded over one process per GPU (rank r of G evaluates the r-th
 * contiguous range, Philox counters = global sample index); each rank runs
 * fdg_accumulate_device into its own acc[R]; ONE collective of R doubles -- RCCL
 * over xGMI -- adds the ranks' partial sums.  No data-path collective exists.
 * The reference has no counterpart (example/benchmark*.jl are single-process).
 * RCCL is bound at run time; without it these calls return FDG_E_NO_DEVICE and
 * everything else keeps working.
 *   rank 0: fdg_comm_unique_id(id) -> ship the 128 bytes to the other ranks by any
 *   means (MPI, a file, torch.distributed) -> every rank, with its device current:
 *   fdg_comm_create(id, rank, world, &c) -> ... fdg_reduce_device(c, d_acc, R, -1, stream). */
#define FDG_COMM_ID_BYTES 128
typedef struct fdg_comm fdg_comm;
int fdg_comm_unique_id(void *id, size_t bytes);
int fdg_comm_create(const void *id, int rank, int world, fdg_comm **out);
int fdg_comm_destroy(fdg_comm *c);
/* d_acc[0..n) <- sum over ranks, in place, on `stream`.  root < 0: every rank gets
 * the sum (all-reduce); else only rank `root` (reduce). */
int fdg_reduce_device(fdg_comm *c, double *d_acc, uint32_t n, int root, void *stream);

/* Integer power used for Power{N}, |N| >= 4 (and N < 0): exposed so host-side
 * checkers can call the very same routine.  Pure host function. */
double fdg_powi(double x, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* FDG_H */
