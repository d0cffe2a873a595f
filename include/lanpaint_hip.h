/* lanpaint_hip.h -- C ABI of liblanpaint_hip.so (MI355X / gfx950).
 *
 * The reference (scraed/LanPaint v2.1.0) has NO native code and NO FFI: its hot
 * path is ~330 lines of eager PyTorch (src/LanPaint/lanpaint.py).  Every entry
 * point below therefore REPLACES a span of eager ATen ops in the reference; the
 * span is cited as file:line (relative to the reference root) on each function.
 * The binding a reference maintainer would add is a ctypes stub -- see
 * INTEGRATION.md and lanpaint_amd/_cabi.py (the one this repo ships).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / ATen types.
 *   - every function returns int: 0 = ok, <0 = LP_E_* (lp_strerror() names it).
 *     No exception crosses the boundary.
 *   - all tensor pointers are DEVICE pointers owned by the caller (torch
 *     allocations).  The library allocates no device memory, keeps no global
 *     state (it reads nothing from the environment; developer switches travel
 *     in lp_step_desc.tune) and is re-entrant.
 *   - every entry point ENQUEUES on the caller's HIP stream and returns without
 *     synchronising, so it may be called while that stream is being captured
 *     into a hipGraph -- with these exceptions, which block the calling thread
 *     and must NOT be called on a capturing stream:
 *       lp_node_call          polls a pinned-host mailbox for the device's answer
 *                             and falls back to hipStreamSynchronize after
 *                             `spin_limit` polls; it also launches hipGraphExec_t
 *                             handles (hipGraphLaunch), which a capture refuses;
 *       lp_replay_call        launches a hipGraphExec_t / updates a graph node's
 *                             arguments (host-side, not capturable);
 *       lp_timer_elapsed_ns   waits for the timed launch (hipEventSynchronize);
 *       lp_graph_*            host-side graph surgery, no stream involved.
 *     lp_timer_create / lp_graph_clone_tail allocate HOST-side runtime handles
 *     (events, a graph clone) that the caller releases with lp_timer_destroy /
 *     lp_graph_release.
 *   - tensors are dense row-major fp32 in the latent's own layout
 *     [B, C, (F), H, W] flattened: n_el = B * el_per_row.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 */
#ifndef LANPAINT_HIP_H
#define LANPAINT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LP_ABI_VERSION 25

/* The library is built with -fvisibility=hidden: the entry points declared LP_API below are its ONLY dynamic symbols (the
 * dispatch functions, kernel handles and device stubs of the C++ side stay internal; tests/test_cabi_exports.py checks
 * `nm -D --defined-only` lists nothing but lp_*). */
#define LP_API __attribute__((visibility("default")))

/* ---- error codes ------------------------------------------------------- */
#define LP_OK             0
#define LP_E_INVALID     -1   /* null / inconsistent argument                  */
#define LP_E_UNSUPPORTED -2   /* layout or flag combination not implemented   */
#define LP_E_LAUNCH      -3   /* hipLaunchKernel failed (hipGetLastError)      */
#define LP_E_ALIGN       -4   /* pointer not aligned for the requested layout */

/* ---- per-row coefficient table ------------------------------------------ */
/* One row of LP_COEF_STRIDE floats per batch row, produced on the device by
 * lp_coeffs() so the think loop needs no host<->device sync (the reference
 * recomputes these ~40 tiny ops + 1 host sync EVERY iteration:
 * lanpaint.py:205,295-328).  Region r: 0 = inpaint ("x" branch, mask==0),
 * 1 = known ("y" branch, mask==1).                                          */
#define LP_COEF_STRIDE   36
#define LP_C_SCALE        0   /* flow: sqrt(abt)+sqrt(1-abt); VE: sqrt(1+sigma^2)  (lanpaint.py:96-99) */
#define LP_C_SQRT_ABT     1
#define LP_C_OMA          2   /* 1 - abt                                         */
#define LP_C_ABT          3
#define LP_C_RSIGMA       4   /* sigma used by the replace step (lanpaint.py:94) */
#define LP_C_DTX          5   /* dt of the inpaint branch  = step                */
#define LP_C_DTY          6   /* dt of the known branch    = beta*step           */
#define LP_C_AX           7   /* 1/(1-abt)          (lanpaint.py:315,319)        */
#define LP_C_AY           8   /* (1+lambda)/(1-abt) (lanpaint.py:316,320)        */
#define LP_C_DX           9   /* sqrt(2)            (lanpaint.py:326)            */
#define LP_C_DY          10
#define LP_C_VALID       11   /* 1.0 if step > 0 else 0.0 (lanpaint.py:205)      */
#define LP_C_REGION0     12   /* 10 floats per region, see LP_R_*                */
#define LP_C_REGION1     22
#define LP_R_E_FULL       0   /* exp(-A dt)                  (lanpaint.py:242)   */
#define LP_R_K_FULL       1   /* (1-exp(-A dt))/A            (lanpaint.py:247)   */
#define LP_R_STD_FULL     2   /* sqrt(D^2 (1-exp(-2A dt))/(2A)) (lanpaint.py:249-252) */
#define LP_R_E_HALF       3   /* same three at dt/2                              */
#define LP_R_K_HALF       4
#define LP_R_STD_HALF     5
#define LP_R_DT           6
#define LP_R_A            7
#define LP_R_CX0          8   /* sqrt(abt)/(1-abt): C = CX0*x0s + CXT*x_t (lanpaint.py:219) */
#define LP_R_CXT          9   /* A - 1/(1-abt)                                   */
#define LP_C_TMODEL      32   /* the time the backbone is called with inside the loop (flow_t or VE sigma,
                                 lanpaint.py:165,170): lets a replayed hipGraph hand `table[:, 32]` to the model */
#define LP_C_RSCALE      33   /* RN(1 / scale), formed in double and rounded once (= the IEEE fp32 quotient 1.0f / scale: a
                                 double has 2 * 24 + 2 <= 53 bits, so the second rounding is innocuous).  The streaming kernels'
                                 flow-model emit x_t / scale divides four elements per lane by this row scalar: with the
                                 correctly rounded reciprocal one residual correction per element gives the IEEE quotient
                                 (lp_common.h::div_shared) -- the reciprocal itself, 11 VALU instructions per lane, now comes
                                 from the table (round 5).                                                             */

typedef struct lp_hyper {
    float    lambda;          /* LanPaint_Lambda   (lanpaint.py:11)             */
    float    beta;            /* LanPaint_Beta     (lanpaint.py:17,188-190)     */
    float    step_size;       /* LanPaint_StepSize (lanpaint.py:14,81)          */
    float    min_step_frac;   /* MinStepFrac       (lanpaint.py:18,81)          */
    int32_t  is_flow;         /* IS_FLUX or IS_FLOW (lanpaint.py:96,144,161)    */
    float    one_plus_lambda; /* fp32(1 + Lambda) with the sum taken in double,
                                 as Python evaluates `(1 + lamb)` (lanpaint.py:183,316) */
} lp_hyper;

/* ---- phases of the fused step kernel -------------------------------------- */
/* The model call is the only unavoidable cut in the loop, so one launch does
 * [everything after model call i] + [everything before model call i+1].      */
#define LP_PH_REPLACE      (1u << 0) /* x = x(1-m)+known*m; x_t = VP(x)   lanpaint.py:94-99           */
#define LP_PH_POST_FIRST   (1u << 1) /* C = coefC; x_t = OU(x_t,dt,C)     lanpaint.py:275-277         */
#define LP_PH_POST_STEADY  (1u << 2) /* C'=coefC; x_t+=(C'-C)dt; x_t=OU(x_t,dt/2,C_old); C=C'  :281-284 */
#define LP_PH_PRE_HALF     (1u << 3) /* x_t = OU(x_t,dt/2,C) -- first half of the NEXT iteration  :280  */
#define LP_PH_EMIT         (1u << 4) /* x_in = model-space(x_t)           lanpaint.py:144-147,163,168 */
#define LP_PH_COEFFS       (1u << 5) /* with LP_PH_REPLACE: this launch ALSO writes the call's coefficient table
                                        (lp_coeffs folded in: one launch less per sigma call) from the raw per-row
                                        times `t_*`; its own replace / emit use the row's scale and replace sigma
                                        computed from the same inputs.  Not with LP_FL_PER_ELEMENT.             */
#define LP_PH_SIGMA        (1u << 6) /* with LP_PH_REPLACE | LP_PH_COEFFS (bit-packed mask): the launch ALSO does what
                                        lp_sigma_times does -- sigma -> (VE sigma, abt, flow t) per row, the two scalars
                                        of the inner-step rule, the rule itself against a speculated count, the mailbox
                                        (lp_step_desc.sg_*) -- and takes its per-row times from sigma instead of t_ve /
                                        t_abt / t_rsig / t_model.  One launch less on a speculated sigma call, where the
                                        later arrival of the answer costs nothing (lp_node_call).                       */

/* ---- flags ---------------------------------------------------------------- */
#define LP_FL_FLOW          (1u << 0)  /* flow/flux VP scaling, else VE                        */
#define LP_FL_MASK_DENOISE  (1u << 1)  /* mask buffer is ComfyUI's denoise_mask: kernel applies
                                          m = 1 - (dm > 0.5)              (nodes.py:281-283)  */
#define LP_FL_MASK_U8       (1u << 2)  /* mask buffer is uint8 0/1 (1 = known)                 */
#define LP_FL_WRITE_X0S     (1u << 3)  /* also store x0s (LangevinState.x0; early stop)        */
#define LP_FL_X0_BF16       (1u << 4)  /* x0 / x0_big are bf16                                 */
#define LP_FL_X0_F16        (1u << 5)  /* x0 / x0_big are fp16                                 */
#define LP_FL_XIN_BF16      (1u << 6)  /* x_in is written as bf16                              */
#define LP_FL_XIN_F16       (1u << 7)  /* x_in is written as fp16                              */
#define LP_FL_PER_ELEMENT   (1u << 8)  /* abt_el/ve_el/... per-element times (AV packs,
                                          lanpaint.py:60-74): general path                     */
#define LP_FL_CFG_FUSED     (1u << 10) /* `x0` = cond prediction, `x0_big` = uncond prediction of ONE batched
                                          backbone pass; the kernel forms both CFG heads itself,
                                          head = uncond + (cond - uncond) * scale  (nodes.py:161-175 +
                                          ComfyUI cfg_function) instead of 2 x 3 eager elementwise passes */
#define LP_FL_MASK_BITS     (1u << 11) /* mask buffer is bit-packed latent_mask (1 = known): element i is
                                          bit (i & 31) of 32-bit word (i >> 5), as lp_pack_mask writes it;
                                          0.125 B/element instead of 4.  Not combinable with MASK_DENOISE /
                                          MASK_U8; binary masks only (SURVEY 8b `mask_kind`)            */
#define LP_FL_NO_REGION_SKIP (1u << 12) /* stream x0, x0_big and y for every element even where the bit-packed mask makes
                                          one of them unused for a whole wave (measurement / A-B switch)       */
#define LP_FL_ES            (1u << 13) /* the POST phase of this launch also evaluates the inner early-stop rule ON THE DEVICE
                                          (earlystop.py:238-336): every block forms the sums of the weighted MSEs (x0s against the
                                          previous x0s and against the drift anchor; iteration 0: x_t after against x_t before)
                                          and adds them into the accumulator set of the iteration (es_partials);
                                          lp_step then enqueues a one-wave kernel that totals the set in a fixed order, applies
                                          the threshold / patience / drift-anchor logic, updates lp_es_state and posts the
                                          trace record to `es_host` (a gated loop instead applies the rule at the top of its
                                          NEXT launch, at any grid size, and enqueues that kernel after the last launch
                                          only).  Row-table launches only (not LP_FL_PER_ELEMENT).                         */
#define LP_FL_ES_GATED      (1u << 14) /* with LP_FL_ES, a launch of a loop the host does not watch (hipGraph replay): once
                                          lp_es_state.stopped is set the launch only re-emits x_in from the committed x_t;
                                          otherwise PRE_HALF is TENTATIVE -- x_t is stored in its post-iteration state, the
                                          state after the half-step goes to es_xte and feeds x_in -- and a POST_STEADY
                                          launch starts from es_xte, so stopping after iteration i leaves exactly the
                                          reference's state after i iterations (round 3 redid the half-step from the same
                                          noise instead of storing it: a second Philox block per element).               */
#define LP_FL_ES_CLOSE      (1u << 15) /* with LP_FL_ES_GATED on the LAST launch of a loop (es_index + 1 == es_n_steps) whose
                                          verdict is folded into the launches (small grids): no closing decision kernel
                                          follows.  The launch, having applied the verdict of the iteration before, accounts
                                          its own iteration (n_ran, total_ran) and posts the call's "done" word itself; the
                                          verdict of the last iteration is never formed -- stopping after the last iteration
                                          changes nothing (earlystop.py:313 only breaks a loop that is over) -- and its trace
                                          record is not written, so a caller that wants the full trace leaves the flag off.  */
#define LP_FL_ES_RING_BITS  (1u << 16) /* with LP_FL_ES and LP_FL_MASK_BITS: es_ring is the BIT-PACKED ring (lp_pack_mask of lp_boundary_ring's
                                          output; bit = ring pixel).  With a hard mask the ring weight is 0 or 1 (ring pixels are
                                          inpaint pixels: 1 - m = 1), so the launch reads 0.125 B / element for it and derives the
                                          weight in registers.  The phase-specialised hard-mask kernels take only this form; an fp32
                                          ring next to a bit-packed mask runs through the run-time kernels.                          */
#define LP_FL_AV            (1u << 17) /* AV packs (MiniMax-H3 flat audio / video latents; lanpaint.py:60-74): every element runs on one of
                                          TWO per-row time sets, chosen by a 0/1 indicator.  `coef` then holds two rows per batch row
                                          (2 r: video times, 2 r + 1: audio times; lp_coeffs with 2 * rows inputs), `av_bits` the
                                          bit-packed indicator (1 = audio; lp_pack_mask layout) and `av_frac` the share of audio
                                          elements.  A wave whose elements all sit on one stream runs the ordinary table path on
                                          that stream's row -- no per-element transcendental, where the reference-shaped
                                          LP_FL_PER_ELEMENT form needs three full-size time tensors and evaluates exp / expm1 per
                                          element; only the wave straddling the seam of a row uses the per-element formulas.
                                          Not with LP_PH_COEFFS / LP_FL_PER_ELEMENT.  (With LP_FL_ES_GATED a stopped launch
                                          re-emits every element with its own stream's scale.)                                 */
#define LP_FL_X0S_GIVEN     (1u << 9)  /* `x0` already holds x0s = x_t + score(x_t) (public
                                          langevin_dynamics(x_t, score, ...) entry, lanpaint.py:192,218) */

/* Device-side state of the inner early stop (one per engine and device; lp_step_desc.es).  Reset by the launch
 * that carries `es_reset` (the replace launch of a sigma call), updated by the deciding block of every
 * LP_FL_ES launch.  x0s_buf: three rotating buffers for LangevinState.x0 -- the stopper compares the current one
 * with the previous one and with the drift anchor (earlystop.py:283-306), so the buffer being written is always
 * the one that is neither.                                                                                      */
typedef struct lp_es_state {
    int32_t  stopped;         /* 1 once patience_counter >= patience_eff (earlystop.py:313)              */
    int32_t  counter;         /* patience_counter                                                       */
    int32_t  n_ran;           /* iterations whose result is committed in x_t / C                        */
    int32_t  cur_slot;        /* x0s_buf index of the last committed iteration's x0s, -1 = none yet     */
    int32_t  anchor_slot;     /* x0s_buf index of the drift anchor, -1 = none                           */
    int32_t  write_slot;      /* x0s_buf index the next POST writes                                     */
    uint32_t reserved0;
    int32_t  enabled;         /* threshold_eff > 0 (earlystop.py:111-113); the zero-inpaint-weight test
                                 (:115-117) is applied when the sums are known                          */
    int64_t  seq_base;        /* mailbox sequence base of the call in flight (set at reset)             */
    int64_t  total_ran;       /* iterations committed since the state was created (never reset): lets a
                                 host that does not wait after every call account them later             */
    double   threshold_eff;   /* threshold * clamp01(4 abt (1 - abt)), abt = mean over rows             */
    double   abt_val;
    float*   x0s_buf[3];
} lp_es_state;

/* Mailbox (`es_host`, pinned host or device memory, doubles): [0] sequence word (int64 bits, stored last with a
 * system-scope release): seq_base + i + 1 after the decision of iteration i, seq_base + LP_ES_SEQ_DONE after the
 * last launch of a gated loop; [1] n_ran, [2] stopped, [3] enabled, [4] threshold_eff, [5] abt_val, [6] total_ran;
 * [LP_ES_TRACE0 + 8 i ..]: record of iteration i = { dist, dist_inpaint, dist_ring, dist_drift (NaN = not
 * evaluated), patience_counter, stopped, 0, 0 }.                                                       */
#define LP_ES_ACC_SLOTS  64
#define LP_ES_ACC_SETS   3
#define LP_ES_ACC_DOUBLES (LP_ES_ACC_SETS * LP_ES_ACC_SLOTS * 8)
#define LP_ES_SEQ_DONE   0x10000
#define LP_ES_TRACE0     8
#define LP_ES_MAILBOX_DOUBLES(n_steps) (LP_ES_TRACE0 + 8 * (n_steps))

/* in-kernel noise generators */
#define LP_RNG_PHILOX 0   /* Philox2x32-10 per element, one Box-Muller pair per launch (independent stream)  */
#define LP_RNG_TORCH  1   /* the device's torch.randn stream, reproduced exactly                             */

/* replace-step source (lanpaint.py:84-94) */
#define LP_REPLACE_KNOWN    0   /* `known` = model_sampling.noise_scaling(...) computed by the caller */
#define LP_REPLACE_VE       1   /* y + n*sigma                                                        */
#define LP_REPLACE_FLOW     2   /* sigma*(noise_scale*n) + (1-sigma)*y                                */

typedef struct lp_step_desc {
    int64_t   n_el;            /* total latent elements                                   */
    int64_t   el_per_row;      /* elements per batch row (C*(F)*H*W), < 2^31               */
    int32_t   rows;            /* B                                                       */
    uint32_t  phases;          /* LP_PH_*                                                 */
    uint32_t  flags;           /* LP_FL_*                                                 */
    int32_t   replace_kind;    /* LP_REPLACE_*                                            */
    float     lambda;          /* duplicated from lp_hyper for the per-element path       */
    float     one_plus_lambda;
    float     beta;
    float     step_size;
    float     min_step_frac;
    float     noise_scale;     /* model_sampling.noise_scale (lanpaint.py:91)             */
    float     cfg_scale;       /* LP_FL_CFG_FUSED: cond_scale      (head 0, x0)           */
    float     cfg_scale_big;   /*                  cond_scale_BIG  (head 1, x0_BIG)       */
    const float* coef;         /* [rows][LP_COEF_STRIDE] from lp_coeffs()                 */
    const float* x;            /* REPLACE: sampler latent (model space)                   */
    const float* known;        /* REPLACE, LP_REPLACE_KNOWN                               */
    const float* noise;        /* REPLACE, VE/FLOW kinds                                  */
    const float* y;            /* latent_image (clean known latent)                       */
    const void*  mask;         /* fp32 (default), u8 or bit-packed (LP_FL_MASK_*), full latent shape */
    float*       x_t;          /* VP-space state, read+written                            */
    float*       C;            /* LangevinState.C, read+written                           */
    float*       x0s;          /* LangevinState.x0 out (LP_FL_WRITE_X0S) or NULL          */
    const void*  x0;           /* model output head 0                                     */
    const void*  x0_big;       /* model output head 1 (may alias x0)                      */
    void*        x_in;         /* EMIT: model-space latent for the next model call        */
    const float* xi_post;      /* host-supplied N(0,1) for POST_* (NULL => generated in-kernel, rng_kind) */
    const float* xi_pre;       /* host-supplied N(0,1) for PRE_HALF (NULL => generated in-kernel)         */
    uint64_t     rng_seed;     /* generator seed / key                                    */
    uint64_t     rng_offset;   /* LP_RNG_PHILOX: launch sequence number (unique per launch);
                                  LP_RNG_TORCH: torch philox offset of this launch's first draw */
    const uint64_t* rng_offset_ptr; /* optional device u64[2] (graph replay): [0] is added to rng_offset;
                                  LP_RNG_TORCH also takes the seed from [1]              */
    const float* abt_el;       /* LP_FL_PER_ELEMENT: per-element abt                      */
    const float* ve_el;        /*                    per-element VE sigma                 */
    const float* rsig_el;      /*                    per-element replace sigma            */
    const float* corr_el;      /* audio_correction (lanpaint.py:173-180) or NULL          */
    /* LP_PH_COEFFS: the inputs of lp_coeffs (same meaning, same strides) and the table to write */
    const float* t_ve;         /* [rows] VE sigma (NULL for flow)                         */
    const float* t_abt;        /* [rows] abt                                              */
    const float* t_rsig;       /* [rows] replace sigma                                    */
    const float* t_model;      /* [rows] backbone time argument -> slot LP_C_TMODEL       */
    float*       coef_out;     /* [rows][LP_COEF_STRIDE]                                  */
    int32_t      t_ve_stride, t_abt_stride, t_rsig_stride, t_model_stride;   /* 0 = broadcast row 0 */
    /* In-kernel noise generator (xi_post / xi_pre NULL).  LP_RNG_TORCH reproduces, bit for bit, the values
     * `torch.randn_like(x_t)` would return on this device for generator state (rng_seed, offset): ATen's
     * Philox4x32-10 thread / offset mapping (DistributionTemplates.h) over rocRAND's own normal4.  Draw order
     * inside one launch: the POST draw, then the PRE draw (offset + rng_inc) -- the reference's order
     * (lanpaint.py:277,280,283).  rng_bg = block * grid of ATen's launch for n_el elements, rng_inc = the
     * generator-offset increment of one such call.                                                        */
    int32_t      rng_kind;     /* LP_RNG_PHILOX (0) | LP_RNG_TORCH (1)                     */
    uint32_t     rng_bg;
    uint32_t     rng_inc;
    /* LP_PH_COEFFS launches of a replayed graph publish the caller's generator state for the captured launches:
     * rng_state_out[0] = rng_state_val[0] (offset base), [1] = rng_state_val[1] (seed); NULL = nothing.      */
    uint64_t*    rng_state_out;
    uint64_t     rng_state_val[2];
    /* Per-call I/O pointers for launches CAPTURED in a hipGraph (their kernargs are frozen at capture): the first
     * lane of the launch stores io_table_val[0..1] to io_table_out[0..1] (NULL = nothing).  The engine's replace
     * launch -- the one launch of a sigma call that stays outside the graph -- publishes { address of the sampler
     * latent x (lanpaint.py:156 writes it in place), address of this call's `out` } for the captured lp_finalize
     * (lp_final_desc.io_table), so that the caller's tensors never have to be staged through static buffers.
     * io_table_out[2] is the "this sigma call is valid" word, see io_valid below.                              */
    uint64_t*    io_table_out;
    uint64_t     io_table_val[2];
    /* Inner early stop on the device (LP_FL_ES; earlystop.py:58-336 with the default metric).                 */
    lp_es_state* es;             /* device state, TWO consecutive lp_es_state (a gated loop on a small grid alternates
                                    between them); also given to the launch that resets it                     */
    float*       es_x0s[3];      /* the three rotating x0s buffers (== es->x0s_buf, as launch arguments so the kernel
                                    selects one by slot index instead of chasing a pointer through the state)     */
    const float* es_ring;        /* mask-edge ring weight (lp_boundary_ring; 4-D latents) as fp32, or bit-packed with
                                    LP_FL_ES_RING_BITS, or NULL                                              */
    double*      es_partials;    /* device scratch, LP_ES_ACC_DOUBLES doubles: the accumulator sets the blocks of an
                                    LP_FL_ES launch add their six sums into (set = es_index mod LP_ES_ACC_SETS, slot =
                                    block mod LP_ES_ACC_SLOTS).  The es_reset launch clears all of it; launch i clears
                                    the set of iteration i + 1.  Ordinary (coarse-grained) device memory: the adds are
                                    hardware fp64 atomics, which fine-grained / host-coherent allocations do not honour */
    double*      es_host;        /* mailbox, LP_ES_MAILBOX_DOUBLES(es_n_steps) doubles                       */
    double       es_threshold;   /* threshold before the abt scaling (earlystop.py:78-81)                    */
    int64_t      es_seq_base;    /* es_reset: sequence base of this call                                     */
    int32_t      es_patience_eff;/* max(1, patience) + 1 (earlystop.py:103)                                  */
    int32_t      es_index;       /* iteration i this launch's POST belongs to                                */
    int32_t      es_n_steps;     /* iterations of the loop (the last launch of a gated loop posts "done")    */
    int32_t      es_reset;       /* 1: this launch (a replace launch) initialises *es for a new call         */
    /* Profiling builds only (library compiled with -DLP_SHADER_CLOCK, scripts/shader_clock.py): thread 0 of the
     * first and of the last block store LP_CLK_STAMPS shader-clock stamps each (s_memtime ticks since its own kernel
     * entry) at clk_out[0..] and clk_out[16..], then the 100 MHz s_memrealtime span of the kernel at [15] / [31].
     * A release build ignores the field.                                                                      */
    /* LP_PH_SIGMA (see there): the arguments of lp_sigma_times_mailbox and of the inner-step rule                */
    const float* sg_sigma;       /* device [rows]                                                              */
    const float* sg_schedule;    /* device [sg_schedule_len]                                                   */
    float*       sg_times_out;   /* device [3][rows]                                                           */
    float*       sg_scalars_out; /* pinned host float[4]                                                       */
    int32_t*     sg_seq_out;     /* pinned host                                                                */
    uint64_t*    sg_valid_out;   /* device word lp_finalize checks                                             */
    double       sg_min_step_frac;
    int32_t      sg_schedule_len, sg_seq, sg_n_steps, sg_early_stop, sg_total_steps, sg_guess;
    double*      clk_out;
    const void*  av_bits;        /* LP_FL_AV: bit-packed stream indicator, 1 = audio element (LP_MASK_BITS_BYTES(n_el) bytes)          */
    float        av_frac;        /* LP_FL_AV: audio elements / all elements (the early-stop threshold uses the mean of the blended abt) */
    uint32_t     reserved2;
    float*       es_xte;         /* LP_FL_ES_GATED: n_el floats, the state after the TENTATIVE first half-step of the next
                                    iteration (lanpaint.py:280).  A gated launch stores it next to the committed x_t; the next
                                    launch of the loop starts from it, a stopped loop never looks at it again.             */
    uint32_t     tune;           /* LP_TUNE_*: developer switches of this launch (micro-benchmarks, A/B runs); 0 in production */
    uint32_t     io_valid;       /* with io_table_out: 1 = this launch also stores 1 into io_table_out[2], the word whose 0 voids a
                                    captured lp_finalize.  Every replace launch that is not part of a speculated lp_node_call sets
                                    it, so that a speculated run which voided itself and was then abandoned (an error return) cannot
                                    leave later replays voided; lp_node_call clears it on the launches it queues itself -- there
                                    the sigma rule owns the word.                                                              */
} lp_step_desc;
#define LP_TUNE_VEC1          (1u << 0)   /* one element per lane whatever the size                                          */
#define LP_TUNE_VEC4          (1u << 1)   /* four elements per lane whenever layout and alignment allow                      */
#define LP_TUNE_ES_NO_DECIDE  (1u << 2)   /* LP_FL_ES: do not enqueue the one-wave decision kernel behind the launch         */
#define LP_TUNE_ES_NO_FOLD    (1u << 3)   /* LP_FL_ES_GATED: decision kernel after every launch instead of the folded verdict */
#define LP_TUNE_ES_NO_ATOMICS (1u << 4)   /* LP_FL_ES: the blocks do not add their sums to the accumulator set (WRONG verdicts: a
                                             measurement switch that prices the atomics)                                    */
#define LP_CLK_STAMPS 9  /* 0 entry, 1 operand loads issued, 2 noise generated, 3 operands arrived, 4 stop verdict
                            formed, 5 arithmetic done, 6 stores issued, 7 per-block sums written, 8 generator started:
                            counter and seed in registers (one-element-per-lane launches)                      */

typedef struct lp_final_desc {
    int64_t   n_el;
    uint32_t  flags;           /* LP_FL_MASK_*, LP_FL_X0_BF16/F16 (dtype of model_out), LP_FL_CFG_FUSED */
    float     cfg_scale;       /* LP_FL_CFG_FUSED: head 0 = uncond + (model_out - uncond)*cfg_scale */
    const void*  model_out;    /* final denoise, head 0 (lanpaint.py:151-153); cond prediction when fused */
    const void*  uncond;       /* LP_FL_CFG_FUSED: uncond prediction, else NULL           */
    const float* y;
    const void*  mask;
    const float* x_src;        /* final model-space x (the last EMIT)                     */
    float*       x_dst;        /* sampler latent, overwritten IN PLACE (lanpaint.py:156); NULL = skip */
    float*       out;          /* out*(1-m) + y*m (lanpaint.py:154)                       */
    uint64_t*    rng_bump_ptr; /* optional: *ptr += rng_bump after the launch (graph replay) */
    uint64_t     rng_bump;
    const uint64_t* io_table;  /* optional device u64[3] (a finalize captured in a hipGraph; word 2 = 0 voids the launch --
                                  nothing written, rng_bump not applied -- and must be 1 otherwise; BOTH published addresses must
                                  be 16-byte aligned -- the launch is laid out for 16 B per lane before it can see
                                  them): x_dst and out are
                                  read from io_table[0] / io_table[1] on the device, as the replace launch of the
                                  same sigma call published them (lp_step_desc.io_table_out); the x_dst / out
                                  fields are then ignored.  A zero address in slot 0 skips the write-back.      */
} lp_final_desc;

/* ---- entry points --------------------------------------------------------- */
LP_API int lp_abi_version(void);
LP_API const char* lp_strerror(int code);

/* K1  per-row coefficient table on the device.
 * Replaces: KSamplerX0Inpaint scalars feeding LanPaint.LanPaint (lanpaint.py:81-82),
 *           prepare_step_size (lanpaint.py:295-328) and the closed-form OU
 *           factors of advance_time_overdamped (lanpaint.py:241-252).
 * ve_sigma / abt / replace_sigma: device fp32, `rows` entries each, or 1 entry
 * broadcast when the matching *_stride is 0.  step_override (nullable): explicit
 * per-row step size (the `step_size` argument of the public langevin_dynamics,
 * lanpaint.py:192) instead of StepSize*max(1-abt, MinStepFrac).  t_model (nullable):
 * copied into slot LP_C_TMODEL.                                                */
LP_API int lp_coeffs(const lp_hyper* hyper, const float* ve_sigma, int ve_stride, const float* abt, int abt_stride,
              const float* replace_sigma, int rs_stride, const float* step_override, int step_stride,
              const float* t_model, int t_stride, int rows, float* coef_table, void* stream);

/* One sigma call's whole enqueue sequence in ONE host call, for callers that replay the think loop as a
 * hipGraph (the loop between the replace step and the finalise, captured by the caller):
 *     [lp_coeffs(...)] ; lp_step(replace) ; hipGraphLaunch(graph_exec, stream) ; lp_finalize(final).
 * `hyper` NULL skips the separate lp_coeffs launch (the replace descriptor then carries LP_PH_COEFFS);
 * `final` NULL skips the lp_finalize launch (it is a node of the captured graph, lp_final_desc.io_table);
 * `replace` NULL skips the replace launch (the caller enqueued it earlier: KSamplerX0Inpaint starts a sigma call
 * before it knows the inner-step count and picks the graph afterwards).
 * Host-side launch cost matters at SDXL-latent sizes (the whole call is ~40 us of GPU time): four trips through
 * an FFI cost more than the kernels they start.  `graph_exec` is a hipGraphExec_t (NULL: skip the graph launch).
 * Stops at the first failing step and returns its code.                                              */
typedef struct lp_call_desc {
    const lp_hyper*      hyper;
    const float*         ve_sigma;      int32_t ve_stride;
    const float*         abt;           int32_t abt_stride;
    const float*         replace_sigma; int32_t rs_stride;
    const float*         t_model;       int32_t t_stride;
    int32_t              rows;
    float*               coef_table;
    const lp_step_desc*  replace;       /* LP_PH_REPLACE | LP_PH_EMIT launch, or NULL           */
    void*                graph_exec;    /* hipGraphExec_t of the captured think loop, or NULL   */
    const lp_final_desc* final;         /* lp_finalize descriptor, or NULL                      */
    const struct lp_graph_binding* replace_binding;
                                        /* non-NULL: the replace launch is the FIRST NODE of `graph_exec`
                                           (lp_graph_bind_replace): `replace` is not launched, its pointers and
                                           scalars are written into that node's arguments
                                           (hipGraphExecKernelNodeSetParams) before the graph launch -- the whole
                                           sigma call is then ONE hipGraphLaunch with nothing eager in front       */
} lp_call_desc;
LP_API int lp_replay_call(const lp_call_desc* call, void* stream);

/* One hipGraphLaunch per sigma call (round 3).  A sigma call captured WITH its replace launch (lanpaint.py:81-99,
 * the first node of the graph) needs that node's per-call arguments -- the sampler's x, the noise, sigma / times,
 * this call's `out`, generator state -- refreshed before every replay.  lp_graph_bind_replace finds the node in the
 * captured hipGraph_t (its single root; checked against the captured descriptor) and records what
 * hipGraphExecKernelNodeSetParams needs; lp_replay_call then patches instead of launching (replace_binding).
 * hipGraphExecKernelNodeSetParams only affects launches enqueued AFTER it (checked on the MI355X with the GPU held
 * busy: scripts/experiments/graph_setparams.hip), so calls may be queued back to back.
 * lp_graph_clone_tail: the same graph WITHOUT that first node, instantiated -- for a caller that enqueues the replace
 * launch early (KSamplerX0Inpaint does not know the inner-step count yet, nodes.py:286-299) and the rest afterwards.
 * lp_graph_release destroys what lp_graph_clone_tail returned.                                                  */
typedef struct lp_graph_binding {
    void*    node;                      /* hipGraphNode_t of the captured replace launch                           */
    void*    func;                      /* its kernel                                                              */
    uint32_t grid[3], block[3];
    uint32_t shared_bytes;
    uint32_t reserved0;                 /* 0 (was a hash of the captured descriptor): a rewrite is checked against the kernel,
                                           grid and block above instead -- the one the replace descriptor dispatches to must
                                           be exactly this launch, or the rewrite is refused (LP_E_INVALID)              */
} lp_graph_binding;
LP_API int lp_graph_bind_replace(void* graph, const lp_step_desc* captured_replace, lp_graph_binding* out);
LP_API int lp_graph_clone_tail(void* graph, void** tail_graph_out, void** tail_exec_out);
LP_API int lp_graph_release(void* tail_graph, void* tail_exec);
/* For the sampler callable (KSamplerX0Inpaint, nodes.py:229-315), which needs the device's word on the inner-step count inside
 * every sigma call: a copy of the captured call `graph` (root = the replace launch, LP_PH_REPLACE | LP_PH_EMIT | LP_PH_COEFFS)
 * whose root is the SAME launch with the sigma algebra folded in (`with_sigma`: the captured replace descriptor with
 * LP_PH_SIGMA and its sg_* fields set), instantiated.  `binding_out` names the new root for lp_node_call's per-call argument
 * refresh.  The captured root must run the launch `with_sigma` without LP_PH_SIGMA dispatches to (LP_E_UNSUPPORTED
 * otherwise); a descriptor lp_step would refuse is refused with the same code before the graph is touched.  Host-side
 * graph surgery only, no stream involved.  Release with lp_graph_release.                                        */
LP_API int lp_graph_clone_sigma_root(void* graph, const lp_step_desc* with_sigma, void** graph_out, void** exec_out,
                                     lp_graph_binding* binding_out);

/* K1a  sigma -> (VE_sigma, abt, flow_t) per batch row plus the two scalars the inner-step rule needs,
 * in ONE launch.  Replaces the ~15 eager scalar ops + 2 host syncs of KSamplerX0Inpaint.__call__
 * (nodes.py:242-252 times, :286 argmin over the schedule, :299 mean(1 - abt)); every operation is a
 * separately rounded fp32 op in the reference's order (no FMA contraction), so n_eff decisions match.
 * times_out: [3][rows] = VE_sigma, abt, flow_t.  scalars_out: [2] = { index of the schedule entry
 * closest to mean(sigma) (first minimum), mean(1 - abt) }.                                        */
LP_API int lp_sigma_times(const float* sigma, int32_t rows, const float* schedule, int32_t schedule_len, int32_t is_flow,
                   float* times_out, float* scalars_out, void* stream);
/* Same launch with a mailbox: `scalars_out` may be device-visible PINNED HOST memory; after the two scalars the
 * kernel stores `seq` to `seq_out` with a system-scope release, so a host thread polling *seq_out learns the two
 * numbers ~2 us after the kernel ran instead of through a blocking device->host copy (the one host dependency of
 * the per-sigma inner-step rule, nodes.py:286-299: sigma exists only on the device, in stream order).       */
LP_API int lp_sigma_times_mailbox(const float* sigma, int32_t rows, const float* schedule, int32_t schedule_len, int32_t is_flow,
                           float* times_out, float* scalars_out, int32_t* seq_out, int32_t seq, void* stream);

/* The sampler-facing callable's steady state in ONE host call (round 3).  KSamplerX0Inpaint.__call__ (nodes.py:229-315)
 * has to learn from the device where sigma sits in the schedule before it can fix the inner-step count (nodes.py:286-299).
 * lp_node_call enqueues lp_sigma_times_mailbox and the replace launch of the call, polls the pinned mailbox for the two
 * scalars, applies the reference's rule
 *     n_eff = 0                                   if total_steps - step <= early_stop
 *           = n_steps                             if min_step_frac <= 0 or frac >= min_step_frac or n_steps <= 0
 *           = max(0, round_half_even(n_steps * frac / min_step_frac))        otherwise   (Python's round())
 * and launches the graph the caller captured for that count (`exec_by_count[n_eff]`: everything of the sigma call after
 * the replace launch).  Three FFI trips and the Python between them become one; the rule is evaluated in double on the
 * float32 scalars exactly as the Python expression does.  `launched` = 0 when no graph is known for the count (the
 * caller finishes the call itself; the replace launch is already enqueued).  `scalars_out` is float[4]: word 2 is the
 * sequence number (`seq_out`), word 3 the count the device computed.                                              */
typedef struct lp_node_call_desc {
    const float*        sigma;          /* device [rows]                                                          */
    int32_t             rows;
    int32_t             schedule_len;
    const float*        schedule;       /* device [schedule_len]: the sampler's sigmas                            */
    int32_t             is_flow;
    int32_t             seq;            /* sequence word this call posts                                          */
    float*              times_out;      /* device [3][rows]                                                       */
    float*              scalars_out;    /* PINNED HOST float[4]: { step index, mean(1 - abt), (seq), device n_eff } */
    int32_t*            seq_out;        /* PINNED HOST                                                            */
    const lp_step_desc* replace;        /* the call's replace launch (LP_PH_REPLACE | ...), NULL = none           */
    int32_t             n_steps;        /* PaintMethod.n_steps (LanPaint_NumSteps)                                */
    int32_t             early_stop;     /* LanPaint_EarlyStop                                                     */
    int32_t             total_steps;    /* len(sigmas) - 1                                                        */
    int32_t             n_counts;       /* entries of exec_by_count                                               */
    double              min_step_frac;  /* LanPaint_MinStepFrac                                                   */
    void* const*        exec_by_count;  /* hipGraphExec_t per inner-step count, NULL entries allowed              */
    int32_t             spin_limit;     /* polls before falling back to hipStreamSynchronize                      */
    int32_t             guess;          /* >= 0: SPECULATE -- queue exec_by_count[guess] before the device has answered;
                                           the sigma kernel evaluates the same rule, and when the true count differs it
                                           zeroes *valid_word, which voids the queued run (its lp_finalize writes
                                           nothing, lp_final_desc.io_table word 2); lp_node_call then queues the call
                                           again for the true count.  < 0: wait for the answer first              */
    uint64_t*           valid_word;     /* device word the captured lp_finalize checks (io_table + 2), or NULL: never
                                           speculate                                                              */
    int32_t             fold_sigma;     /* 1: a speculated call carries the sigma algebra inside its replace launch
                                           (LP_PH_SIGMA) instead of a kernel of its own, when the descriptor allows */
    int32_t             n_eff;          /* out                                                                    */
    int32_t             launched;       /* out: 1 = exec_by_count[n_eff] was launched                             */
    int32_t             speculated;     /* out: 1 = a run was queued for `guess`                                  */
    int32_t             hit;            /* out: 1 = ... and the guess was right                                   */
    float               step_f, frac;   /* out: the two scalars as read from the mailbox                          */
    void* const*        full_exec_by_count;
                                        /* optional, per inner-step count like exec_by_count: hipGraphExec_t of the WHOLE sigma
                                           call whose first node is the replace launch with the sigma algebra folded in
                                           (lp_graph_clone_sigma_root).  A speculated call then is ONE hipGraphLaunch: the
                                           node's arguments are refreshed from `replace` + the sigma fields of this
                                           descriptor (hipGraphExecKernelNodeSetParams), nothing is launched in front of
                                           the graph.  NULL / NULL entry: the replace launch goes eagerly in front of
                                           exec_by_count[guess] as before                                           */
    const struct lp_graph_binding* const* full_binding_by_count;   /* the root node of each full_exec_by_count entry */
    int32_t             one_launch;     /* out: 1 = the speculated call went out as one graph launch              */
    int32_t             reserved0;
} lp_node_call_desc;
LP_API int lp_node_call(lp_node_call_desc* call, void* stream);
/* the rule alone (host arithmetic; tests pin it against the reference's min_step_frac_effective_steps table)   */
LP_API int32_t lp_effective_inner_steps(int32_t n_steps, double step_f, double frac, int32_t total_steps, int32_t early_stop,
                                 double min_step_frac);

/* K0 / K_first / K2  the fused step (phases select the work).
 * Replaces: lanpaint.py:94-99 (REPLACE), :159-184 + :212-220 (score split + Coef_C),
 *           :232-254 (exact OU + noise injection), :274-286 (the scheme),
 *           :144-147 / :163 / :168 (EMIT).                                     */
LP_API int lp_step(const lp_step_desc* desc, void* stream);

/* Measurement hooks (bench.py roofline leg): lp_step_timed launches exactly like
 * lp_step but through hipExtLaunchKernelGGL with a start/stop event pair bound to the
 * dispatch itself, so lp_timer_elapsed_ns returns the kernel's own begin->end time
 * (what rocprofv3 --kernel-trace reports), not a host-side interval.  The timer is a
 * caller-owned handle; lp_timer_elapsed_ns blocks until that launch has finished.     */
LP_API int lp_timer_create(void** timer);
LP_API int lp_timer_destroy(void* timer);
LP_API int lp_step_timed(const lp_step_desc* desc, void* stream, void* timer);   /* LP_E_UNSUPPORTED for LP_FL_ES launches */
/* n timed launches of the same descriptor from one host call (rng_offset + i per launch), so the GPU stays
 * busy between them: launched one by one through an FFI the host paces a ~10 us kernel and every dispatch
 * starts on an idle chip (measured 13.0 us instead of the 10.5 us rocprofv3 reports for the same kernel). */
LP_API int lp_step_timed_burst(const lp_step_desc* desc, void* stream, void* const* timers, int32_t n);
LP_API int lp_timer_elapsed_ns(void* timer, double* ns);

/* Measurement utility, like lp_step_timed_burst (bench.py's `launch_floor`; no reference counterpart -- the reference has no
 * launch structure to measure): ONE host call enqueues `repeats` x [ for i in 0 .. n-1: `before` (an lp_step launch, NULL =
 * none), hipGraphLaunch(graph_execs[i]) (NULL entry = none), `after` (an lp_step launch, NULL = none) ] on `stream`.  With the
 * hipGraphExec_t handles of a job's captured sigma calls and an elementwise launch standing for the sampler's update between
 * them, the wall time of the burst is what the schedule costs with NO host code between the launches: the floor a
 * host-driven loop over the same graphs can reach.  Not capture-safe (drives graph handles). */
LP_API int lp_replay_burst(void* const* graph_execs, int32_t n, const lp_step_desc* before, const lp_step_desc* after,
                           int32_t repeats, void* stream);

/* K3  finalise: known-region reprojection + in-place write-back.
 * Replaces: lanpaint.py:154,156.                                               */
LP_API int lp_finalize(const lp_final_desc* desc, void* stream);

/* Standalone N(0,1) fill with the generator the fused kernel uses: Philox2x32-10, one
 * block per latent element keyed on (seed, element, launch offset), Box-Muller; slot 0 =
 * cosine branch (POST stream), 1 = sine branch (PRE stream).  Lets tests reproduce the
 * in-kernel noise exactly.  Replaces torch.randn_like (lanpaint.py:252).               */
LP_API int lp_philox_normal(float* out, int64_t n_el, uint64_t seed, uint64_t offset, uint32_t slot, void* stream);
/* Fill `out` with what torch.randn(n_el, device=...) returns for generator state (seed, offset) on this device
 * (test hook for LP_RNG_TORCH; bg as in lp_step_desc.rng_bg).                                            */
LP_API int lp_torch_normal(float* out, int64_t n_el, uint64_t seed, uint64_t offset, uint32_t bg, void* stream);

/* K4  inner early-stop metric (earlystop.py:32-55).
 * lp_boundary_ring: ring[i] = (mask<=0.5) & any 4-neighbour(H,W) known, as fp32
 *                   (planes = B*C images of H x W).
 * lp_wmse_pair:     acc[0..3] = { sum(w1 d^2), sum(w1), sum(w2 d^2), sum(w2) }
 *                   with d = a - b, w1 = 1 - mask (inpaint weight), w2 = ring
 *                   (NULL => acc[2..3] = 0).  acc is a device double[4]; the
 *                   reduction order is fixed, so results are deterministic.
 *                   block_scratch: device double[4 * scratch_blocks].          */
LP_API int lp_boundary_ring(const float* mask, float* ring, int64_t planes, int32_t height, int32_t width, void* stream);
LP_API int lp_wmse_pair(const float* a, const float* b, const float* mask, const float* ring, int64_t n_el,
                 double* acc, double* block_scratch, int32_t scratch_blocks, void* stream);

/* Bytes of the bit-packed form of an n_el-element mask (whole 64-bit ballot words). */
#define LP_MASK_BITS_BYTES(n_el) ((((n_el) + 63) / 64) * 8)

/* Pack a binary fp32 mask into the LP_FL_MASK_BITS layout: one wave64 ballot per 64 elements.
 * flags = 0: `mask` is latent_mask, bit = (v > 0.5); flags = LP_FL_MASK_DENOISE: `mask` is ComfyUI's
 * denoise_mask, bit = !(v > 0.5) (nodes.py:281-283 folded in).  `bits` holds LP_MASK_BITS_BYTES(n_el)
 * bytes, 8-byte aligned; tail bits are 0.  `nonbinary` (nullable, device int32) is set to 1 when an
 * input value is neither 0 nor 1 (soft mask: the packed form would not be equivalent).             */
LP_API int lp_pack_mask(const float* mask, int64_t n_el, uint32_t flags, void* bits, int32_t* nonbinary, void* stream);
/* Same launch, which also writes the fp32 latent_mask (1 = known; nodes.py:281-283 with LP_FL_MASK_DENOISE) to `latent_out`
 * (n_el floats; may be the same buffer as `mask` when flags == 0 -- the kernel declares neither pointer restrict).  One launch re-derives BOTH forms of a mask whose tensor may have been
 * rewritten in place -- what KSamplerX0Inpaint does on every sigma call for tensors that carry no version counter
 * (torch.inference_mode), where the reference recomputes the mask on every call anyway (nodes.py:277-283).             */
LP_API int lp_pack_mask_latent(const float* mask, int64_t n_el, uint32_t flags, void* bits, float* latent_out, void* stream);

/* ATen's nearest-exact source-index rules (F.interpolate(mode="nearest-exact"): nodes.py:78,88,110,125-127,1079,1278-1287).
 * "Bit-exact mask index math" means the rule of the kernel torch runs on the device the REFERENCE holds the mask on -- the
 * reference resamples before `.to(device)` (nodes.py:159-160), i.e. on the CPU tensor ComfyUI hands it -- and ATen has three
 * (every (in, out) <= 512 checked against torch 2.10 on the CPU: tests/test_oracle_properties.py); scale = float(in)/float(out):
 *   SCALAR           min(int(floorf((i + 0.5f) * scale)), in-1): torch's GPU kernels; CPU 2-D kernel when out_h + out_w <= 128;
 *                    CPU channels-last kernels with > 3 channels
 *   CPU_GENERIC_FMA  s = max(fmaf(scale, i + 0.5f, -0.5f), 0); min(int(floorf(float(double(s) + 0.5))), in-1): the CPU's
 *                    TensorIterator kernel (1-D, 3-D, 2-D with out_h + out_w > 128) as its AVX2 / AVX512 builds contract it
 *   CPU_GENERIC      the same with product and subtraction rounded separately (a CPU without FMA: ATEN_CPU_CAPABILITY=default)
 * The three agree on every down-sampling pair (pixel mask -> latent grid); up-sampling they differ on ties (2 -> 41, i = 20). */
#define LP_NN_ATEN_SCALAR          0
#define LP_NN_ATEN_CPU_GENERIC_FMA 1
#define LP_NN_ATEN_CPU_GENERIC     2
#define LP_RESHAPE_BINARIZE        1      /* lp_reshape_mask flags bit 0: also apply 1 - (v > 0.5) (nodes.py:281-283) */
#define LP_RESHAPE_RULE_SHIFT      8      /* lp_reshape_mask flags bits 8..9: one of LP_NN_ATEN_*                      */

/* K5  mask preparation (nodes.py:59-133); index math bit-for-bit with torch's nearest-exact.
 * dst[b][c][f][h][w] = max over the temporal window (video: 5 taps, -inf pad;
 * else 1 tap) of src[f_src(f+k)][h_src(h)][w_src(w)], with idx_src(i) by the LP_NN_ATEN_* rule in `flags`
 * (0 = the scalar rule: every caller of ABI <= 17 passed 0 or 1 here),
 * with dst batch b reading src batch b % src_b and dst channel c reading src
 * channel c % src_c (the reference's repeat + slice).  `flags`: LP_RESHAPE_BINARIZE | (rule << LP_RESHAPE_RULE_SHIFT). */
LP_API int lp_reshape_mask(const float* src, int32_t src_b, int32_t src_c, int32_t src_f, int32_t src_h, int32_t src_w,
                    float* dst, int32_t batch, int32_t channels, int32_t dst_f, int32_t dst_h, int32_t dst_w,
                    int32_t temporal_taps, int32_t flags, void* stream);

/* Post-decode mask blend (pixel space, once per job):
 *   m = conv2d(max_pool2d(mask, k, stride 1, pad k/2), gaussian_kernel_2d(k), pad k/2)
 *   out = image1 * (1 - m) + image2 * m
 * Replaces MaskBlend.blend_images (nodes.py:610-638) and merge_video_with_mask
 * (nodes.py:1060-1088, incl. its nearest-exact resample of a lower-resolution mask).
 * One fused launch: the mask tile (+ 2*(k/2) halo) is staged in LDS, dilated and blurred
 * separably there (the 2-D Gaussian is the outer product of its normalised 1-D profile),
 * then the NHWC images are blended.  k odd, 1..51.                                       */
typedef struct lp_blend_desc {
    int32_t batch, height, width, channels;   /* images are [batch, height, width, channels] fp32 */
    int32_t k;                                /* blend_overlap                                  */
    int32_t mask_batch;                       /* 1 = one mask frame for every image, else == batch */
    int32_t mask_h, mask_w;                   /* mask resolution (resampled nearest-exact when != image) */
    const float* mask;                        /* [mask_batch, mask_h, mask_w]                   */
    const float* image1;
    const float* image2;
    float*       out;                         /* [batch, height, width, channels]               */
    float*       smooth_out;                  /* optional [batch, height, width] smoothed mask  */
    int32_t nn_rule;                          /* LP_NN_ATEN_* rule of the mask resample (ABI 18) */
    int32_t reserved0;
} lp_blend_desc;
LP_API int lp_mask_blend(const lp_blend_desc* desc, void* stream);

/* ---- video mask editor (reference src/LanPaint/videomask.py, nodes.py:890-995) ----------------------------
 * The reference's LanPaint_VideoMaskEditor builds one mask per video frame on the host: binarise the painted keyframes, a
 * signed distance field per keyframe (scipy's EDT), a translation-compensated SDF blend + sigmoid for the frames between two
 * keyframes, then Pillow's 8-bit BILINEAR up to the video size.  Three jobs here; the host (lanpaint_amd/videomask.py)
 * builds the per-frame plan and the resize coefficients, the device does every per-pixel pass.  Sides are 1..16384
 * (int32 squared distances stay exact); larger sides are LP_E_INVALID.                                                   */
#define LP_VMASK_MAX_SIDE 16384
#define LP_VMASK_D2_NONE  (-1)    /* d2 of a pixel whose plane has no pixel of the wanted kind (empty / full keyframe) */
#define LP_VMASK_ZERO     0       /* lp_vmask_frame.kind: all-zero frame (outside the keyframe window)                */
#define LP_VMASK_KEY      1       /*   a keyframe: its original soft values                                            */
#define LP_VMASK_INNER    2       /*   between keyframes key_lo < t < key_hi: the SDF morph                            */
#define LP_VMASK_OUT_U8   1       /* lp_vmask_morph_desc.flags: write uint8 codes trunc(m * 255.0f) instead of fp32    */

/* EDT + SDF + centroid of n_keys keyframes at once (videomask.py:105-170 _edt_2d / _signed_distance / _centroid).
 *   keys  [n_keys, h, w] fp32; foreground = (v >= 0.5)
 *   d2    out [n_keys, 2, h, w] int32: plane 0 = exact squared Euclidean distance to the nearest foreground pixel, plane 1 to
 *         the nearest background pixel; LP_VMASK_D2_NONE where the keyframe has none
 *   sdf   out [n_keys, h, w] fp64: sqrt(d2_bg) - sqrt(d2_fg); -max(h, w)/2 for an empty keyframe, +max(h, w)/2 for a full one
 *   csum  out [n_keys, 3] uint64: foreground count, sum of its row indices, sum of its column indices (exact; the centroid is
 *         (sum_y / n, sum_x / n)).  Zeroed by this call.                                                                */
typedef struct lp_vmask_edt_desc {
    int32_t n_keys, height, width, reserved0;
    const float* keys;
    int32_t*     d2;
    double*      sdf;
    uint64_t*    csum;
} lp_vmask_edt_desc;
LP_API int lp_vmask_edt(const lp_vmask_edt_desc* desc, void* stream);

/* One output frame of lp_vmask_morph (videomask.py:173-240 interpolate_masks).  INNER: with S(f, dy, dx)(y, x) = f(y - dy,
 * x - dx), 0 outside the frame,  d = omw * S(sdf[key_lo], sy1, sx1) + wf * S(sdf[key_hi], -sy2, -sx2)  in fp64, products and
 * sum rounded separately, then float(1 / (1 + exp(-clip(d, -50, 50)))).  KEY: keys[key_lo].  key_* index the key stack. */
typedef struct lp_vmask_frame {
    int32_t kind, key_lo, key_hi, sx1, sy1, sx2, sy2, reserved0;
    double  wf, omw;
} lp_vmask_frame;

/* The morph over [n_frames, h, w] in one launch (videomask.py:173-240).  frames: device [n_frames]; sdf may be NULL when no
 * frame is INNER.  out: fp32, or uint8 codes with LP_VMASK_OUT_U8 (what resize_masks quantises, videomask.py:58-65).     */
typedef struct lp_vmask_morph_desc {
    int32_t n_frames, n_keys, height, width;
    uint32_t flags;
    int32_t  reserved0;
    const lp_vmask_frame* frames;
    const float*  keys;
    const double* sdf;
    void*         out;
} lp_vmask_morph_desc;
LP_API int lp_vmask_morph(const lp_vmask_morph_desc* desc, void* stream);

/* Pillow's 8-bit BILINEAR resize of uint8 frames (resize_masks, videomask.py:58-65: Image.resize(size, BILINEAR)), output
 * fp32 code / 255.  Horizontal then vertical pass, uint8 in between; per axis the caller's tables from Pillow's
 * precompute_coeffs: bounds [out, 2] = (first source index, tap count), weights [out, ksize] 22-bit fixed point.  An axis
 * whose size does not change takes the identity table (tap weights 1, 0), which equals skipping the pass.               */
typedef struct lp_vmask_resize_desc {
    int32_t n_frames, in_h, in_w, out_h, out_w, ksize_x, ksize_y, reserved0;
    const uint8_t* src;          /* [n_frames, in_h, in_w]   */
    const int32_t* bounds_x;
    const int32_t* weights_x;
    const int32_t* bounds_y;
    const int32_t* weights_y;
    float*         dst;          /* [n_frames, out_h, out_w] */
} lp_vmask_resize_desc;
LP_API int lp_vmask_resize(const lp_vmask_resize_desc* desc, void* stream);

/* ---- AV decode: audio merge (reference nodes.py:1091-1136 merge_audio_with_mask, run by LanPaint_AVDecode,
 * nodes.py:1139-1227) ----------------------------------------------------------------------------------------------------
 * From the point where both waveforms are at the original sample rate (lanpaint_amd/audio.py resamples before the call):
 *   w[i]  = mask[i]                          when mask_len == n (a per-sample mask, soft values allowed)
 *         = mask[src(i)]                     otherwise; src = ATen's nearest-exact 1-D index, rule nn_rule (LP_NN_ATEN_*)
 *   w'[i] = (1/cf) * sum_{k=0}^{cf-1} w[clamp(i - cf/2 + k, 0, n-1)]      when cf > 1 (integer cf/2; any cf >= 1 vs n);
 *           the reference's replicate pad (cf/2, cf-1-cf/2) + conv1d(ones/cf).  Evaluated as float(S * double(1.0f / cf)):
 *           S the window sum in fp64, times the reference's fp32 kernel tap, rounded once.  For a 0/1 mask S is exact and
 *           w' = fl(count * fl(1/cf)).  For soft values S is a difference of two fp64 prefixes of the whole signal and
 *           carries their rounding: |w' - exact| <= ulp32(w') + (mask_len + 4) * 2^-52 * sum_i |w[i]| / cf -- absolute
 *           error far below the reference's own conv1d, but many fp32 ulps of a w' that is itself tiny.  cf <= 1: w' = w.
 *   out[b][c][i] = o * (1 - w') + p * w'     fp32, every product and the sum rounded on its own (no FMA), like torch's ops
 * o = orig[b * orig_sb + c * orig_sc + i], p = inpainted[b * inp_sb + c * inp_sc + i] (element strides; 0 = broadcast: the
 * reference's mono expand and batch broadcasting; orig[:, :Ci] is orig_sc with channels = Ci).  Samples are contiguous in
 * every row; out is [batch, channels, n] contiguous.  The window sum is a difference of the prefix function of the
 * piecewise-constant w, from a (mask_len + 1)-entry fp64 table the call builds in `workspace` (first launch, one workgroup)
 * -- O(1) per sample whatever cf is; one launch then does the weight, the crossfade and the lerp, 4 samples per lane.
 * workspace: LP_AUDIO_WS_BYTES(mask_len) bytes, 8-byte aligned, needed when cf > 1 (NULL allowed otherwise).           */
#define LP_AUDIO_WS_BYTES(mask_len) (12 * ((int64_t)(mask_len) + 1))
typedef struct lp_audio_desc {
    int32_t n;                    /* samples per row, >= 1                                           */
    int32_t mask_len;             /* Fm >= 1: mask values at frame rate (or n: per sample)           */
    int32_t batch, channels;      /* output rows                                                     */
    int32_t cf;                   /* crossfade window in samples; 0 or 1 = none                      */
    int32_t nn_rule;              /* LP_NN_ATEN_* rule of the mask's up-sampling                    */
    int64_t orig_sb, orig_sc;     /* element strides of orig per batch / channel (>= 0)              */
    int64_t inp_sb, inp_sc;       /* element strides of inpainted per batch / channel (>= 0)         */
    const float* mask;            /* [mask_len]                                                      */
    const float* orig;
    const float* inpainted;
    float*       out;             /* [batch, channels, n]                                            */
    void*        workspace;
} lp_audio_desc;
LP_API int lp_audio_merge(const lp_audio_desc* desc, void* stream);

/* ---- Detailer crop / stitch (beyond the reference: its README lists "Detailer" as its open item) --------------------------
 * Inpaint at the resolution of the masked region: find the mask's bounding box, cut a window out of the NHWC image and
 * resample it to a working size, and after sampling resample the result back and blend it into the original through the
 * MaskBlend-smoothed mask.  The host (lanpaint_amd/detail.py) plans the window from the four bbox integers and builds the tap
 * tables; the device does every per-pixel pass.  Sides are 1..LP_DETAIL_MAX_SIDE, channels 1..LP_DETAIL_MAX_CHANNELS.    */
#define LP_DETAIL_MAX_SIDE     32768
#define LP_DETAIL_MAX_CHANNELS 64

/* Bounding box of mask > 0.5 over every plane.
 *   mask  [planes, height, width] fp32
 *   bbox  out, device, 4 x int32 {row_min, row_max, col_min, col_max}, inclusive; {height, -1, width, -1} when no element is
 *         set.  Initialised by this call.  Integer atomics only: the result does not depend on the order of arrival.
 * LP_E_INVALID: null pointer, planes <= 0, a side outside 1..LP_DETAIL_MAX_SIDE; LP_E_UNSUPPORTED: planes > 65535.          */
LP_API int lp_mask_bbox(const float* mask, int32_t planes, int32_t height, int32_t width, int32_t* bbox, void* stream);

/* Window [y0, y0 + win_h) x [x0, x0 + win_w) of src [batch, src_h, src_w, channels] -> dst [batch, out_h, out_w, channels],
 * separable, from the caller's tables: per axis bounds [out, 2] int32 = (first tap relative to the window, tap count) and
 * weights [out, ksize] fp32.  With the tables of torch's antialias rule (detail.aa_coeffs) this is
 * F.interpolate(window, size, mode, align_corners=False, antialias=True); the window's edges are edges, no tap reads outside
 * it (entries are clamped to the window).  Horizontal pass, then vertical, fp32 sums with the taps in ascending order.  Same
 * size in and out copies the window bit for bit and reads no table (the table pointers may be NULL).
 * LP_E_INVALID: null pointer, non-positive size, a side or channel count past the limits, the window outside the image,
 * ksize <= 0; LP_E_ALIGN: dst not 16-byte aligned; LP_E_UNSUPPORTED: batch > 65535.                                         */
typedef struct lp_detail_resample_desc {
    int32_t batch, src_h, src_w, channels;
    int32_t y0, x0, win_h, win_w;
    int32_t out_h, out_w, ksize_x, ksize_y;
    const float*   src;
    const int32_t* bounds_x;
    const float*   weights_x;
    const int32_t* bounds_y;
    const float*   weights_y;
    float*         dst;
} lp_detail_resample_desc;
LP_API int lp_detail_resample(const lp_detail_resample_desc* desc, void* stream);

/* Stitch a detailed window back:  with m = conv2d(max_pool2d(mask, k, 1, k/2), gaussian_kernel_2d(k), pad k/2) over the WHOLE
 * image (lp_mask_blend's smoothed mask),
 *   out = original * (1 - m) + detail * m     inside the window (the arithmetic of lp_mask_blend),
 *   out = original, bit for bit               outside it.
 * Two launches: a streaming copy original -> out, then the window's tiles, each with its mask halo in LDS.  No full-frame
 * temporary; out must not be original.  k odd, 1..51.
 *   mask [mask_batch, height, width], mask_batch 1 or batch; original, out [batch, height, width, channels];
 *   detail [batch, win_h, win_w, channels] (already at the window's size: lp_detail_resample brings it there).
 * LP_E_INVALID: null pointer, out == original, non-positive size, limits, the window outside the image, k even or outside
 * 1..51, mask_batch; LP_E_UNSUPPORTED: batch > 65535.                                                                      */
typedef struct lp_detail_stitch_desc {
    int32_t batch, height, width, channels;
    int32_t y0, x0, win_h, win_w;
    int32_t k, mask_batch;
    const float* mask;
    const float* original;
    const float* detail;
    float*       out;
} lp_detail_stitch_desc;
LP_API int lp_detail_stitch(const lp_detail_stitch_desc* desc, void* stream);

/* ---- Detailer per region (beyond the reference, like the Detailer itself) ------------------------------------------------------
 * Split the mask into its connected areas, detail each in a window of its own, all windows of one size so the crops stack as
 * one sampler batch.  The host (lanpaint_amd/detail.py, plan_regions) groups components into regions from the table below. */
#define LP_DETAIL_MAX_COMPONENTS 4096
#define LP_DETAIL_MAX_REGIONS    64

/* Connected components of  S = {(y, x): mask[p, y, x] > 0.5 for some plane p},  8-connected.  A
 * component's label is 1 + the rank of its smallest flat index y * width + x among all components: labels run 1..n in raster
 * order of first pixel, 0 is background -- scipy.ndimage.label(S, ones((3, 3))).
 *   mask    [planes, height, width] fp32
 *   labels  out, device, int32 [height, width]; exact whatever n is
 *   table   out, device, int32 [1 + 5 * LP_DETAIL_MAX_COMPONENTS]: table[0] = n, the true count even past the cap; for
 *           id = 1 .. min(n, cap), table[1 + 5 * (id - 1) ..] = {row_min, row_max, col_min, col_max, area}, boxes inclusive;
 *           rows past n hold {height, -1, width, -1, 0}
 *   workspace  device, LP_COMPONENTS_WS_BYTES(height, width) bytes, 16-byte aligned: the union-find's parent array and the
 *           prefix sum's per-chunk counts
 * Seven plain launches on `stream` (csrc/label_kernel.hip); integer atomics only, the result does not depend on the order of
 * arrival.  LP_E_INVALID: null pointer, planes <= 0, a side outside 1..LP_DETAIL_MAX_SIDE, a short workspace; LP_E_ALIGN:
 * workspace not 16-byte aligned; LP_E_UNSUPPORTED: planes > 65535.  All checked before any HIP call.                        */
#define LP_COMPONENTS_WS_BYTES(height, width) ((((int64_t)(height) * (width) + 1023) / 1024) * 4100)
LP_API int lp_mask_components(const float* mask, int32_t planes, int32_t height, int32_t width, int32_t* labels,
                              int32_t* table, void* workspace, int64_t workspace_bytes, void* stream);

/* lp_detail_resample for `regions` windows of one size in one call:  dst [regions * batch, out_h, out_w,
 * channels], region-major, dst[r * batch + b] = lp_detail_resample of the window at origins[r] of src[b], bit for bit.
 *   origins  DEVICE int32 [regions, 2] = (y0, x0); an origin is clamped so that its window lies inside the image
 * With `labels` the source is a mask (channels == 1) and region r sees it with foreign components erased:
 *   value = 0 where labels[y, x] != 0 and owner[labels[y, x]] != r + 1 (a label >= owner_len is foreign), the mask's own value
 *   elsewhere -- label 0 (soft values at or below 0.5) is kept.
 *   labels  device int32 [src_h, src_w] (lp_mask_components), or NULL: no erasing;  owner  device int32 [owner_len]
 *   scratch device fp32 [regions * batch * win_h * win_w], 16-byte aligned: the erased windows, needed with `labels` when the
 *           size changes (a window-sized temporary; no frame-sized per-region mask exists anywhere)
 * Errors as lp_detail_resample, plus LP_E_INVALID: regions outside 1..LP_DETAIL_MAX_REGIONS, null origins, labels with
 * channels != 1 or without owner / scratch; LP_E_UNSUPPORTED: regions * batch > 65535.                                      */
typedef struct lp_detail_resample_regions_desc {
    int32_t batch, src_h, src_w, channels;
    int32_t regions, win_h, win_w, owner_len;
    int32_t out_h, out_w, ksize_x, ksize_y;
    const int32_t* origins;
    const float*   src;
    const int32_t* bounds_x;
    const float*   weights_x;
    const int32_t* bounds_y;
    const float*   weights_y;
    float*         dst;
    const int32_t* labels;
    const int32_t* owner;
    float*         scratch;
} lp_detail_resample_regions_desc;
LP_API int lp_detail_resample_regions(const lp_detail_resample_regions_desc* desc, void* stream);

/* lp_detail_stitch composed over regions, in region order:
 *   out_0 = original;   out_{r+1} = lp_detail_stitch(out_r, detail[r], mask_r, window r);   out = out_regions
 * bit for bit, mask_r the mask with foreign components erased as above (labels NULL: the mask itself for every region).
 * Windows may overlap, so the order is part of the result.  One streaming copy original -> out, then one launch per region
 * over its window's tiles, in place on out: one thread reads and writes a given element.
 *   origins  HOST int32 [regions, 2] = (y0, x0), read during the call; every window must lie inside the image
 *   detail   [regions * batch, win_h, win_w, channels], region-major, already at the window's size
 * Errors as lp_detail_stitch, plus LP_E_INVALID: regions outside 1..LP_DETAIL_MAX_REGIONS, null origins, labels without
 * owner.                                                                                                                    */
typedef struct lp_detail_stitch_regions_desc {
    int32_t batch, height, width, channels;
    int32_t regions, win_h, win_w, k;
    int32_t mask_batch, owner_len;
    const int32_t* origins;
    const float*   mask;
    const float*   original;
    const float*   detail;
    float*         out;
    const int32_t* labels;
    const int32_t* owner;
} lp_detail_stitch_regions_desc;
LP_API int lp_detail_stitch_regions(const lp_detail_stitch_regions_desc* desc, void* stream);

/* ---- Detailer that follows a moving mask (beyond the reference, like the Detailer itself) --------------------------------------
 * A video mask moves: the union box of a small subject that crosses the frame is most of the frame.  Here every frame gets a
 * window of its own, all of one size, so the crops still stack as one sampler batch.  The host (lanpaint_amd/detail.py,
 * plan_track) plans the windows' path from one box per frame.                                                                */

/* lp_mask_bbox per plane:  row p of `boxes` is what lp_mask_bbox returns for plane p alone.
 *   mask   [planes, height, width] fp32
 *   boxes  out, device, int32 [planes, 4] = {row_min, row_max, col_min, col_max}, inclusive; {height, -1, width, -1} for a plane
 *          with no element set.  Initialised by this call.
 * One launch over every plane (planes on a grid axis), integer atomics only.  Limits and errors as lp_mask_bbox.            */
LP_API int lp_mask_bbox_frames(const float* mask, int32_t planes, int32_t height, int32_t width, int32_t* boxes, void* stream);

/* lp_detail_resample with a window per image:  dst [batch, out_h, out_w, channels], dst[b] = lp_detail_resample of the window at
 * origins[b] of src[b], bit for bit, in one launch.
 *   origins  DEVICE int32 [batch, 2] = (y0, x0); an origin is clamped so that its window lies inside the image
 * Same size in and out copies the windows bit for bit and reads no tap table.  Errors as lp_detail_resample, plus
 * LP_E_INVALID: null origins.                                                                                                */
typedef struct lp_detail_resample_track_desc {
    int32_t batch, src_h, src_w, channels;
    int32_t win_h, win_w, out_h, out_w;
    int32_t ksize_x, ksize_y;
    const int32_t* origins;
    const float*   src;
    const int32_t* bounds_x;
    const float*   weights_x;
    const int32_t* bounds_y;
    const float*   weights_y;
    float*         dst;
} lp_detail_resample_track_desc;
LP_API int lp_detail_resample_track(const lp_detail_resample_track_desc* desc, void* stream);

/* lp_detail_stitch with a window per image:  out[b] = lp_detail_stitch(original[b], detail[b], mask[b or 0], window at
 * origins[b]), bit for bit; outside image b's window out[b] is original[b] bit for bit.  Two launches whatever the batch: the
 * streaming copy original -> out, then the tiles of every image's window (the image on a grid axis).  Images do not overlap
 * each other, so there is no order to keep.
 *   origins  DEVICE int32 [batch, 2] = (y0, x0), clamped as above
 *   detail   [batch, win_h, win_w, channels], already at the window's size
 * Errors as lp_detail_stitch, plus LP_E_INVALID: null origins.                                                               */
typedef struct lp_detail_stitch_track_desc {
    int32_t batch, height, width, channels;
    int32_t win_h, win_w, k, mask_batch;
    const int32_t* origins;
    const float*   mask;
    const float*   original;
    const float*   detail;
    float*         out;
} lp_detail_stitch_track_desc;
LP_API int lp_detail_stitch_track(const lp_detail_stitch_track_desc* desc, void* stream);

/* ---- Detailer per subject of a video (beyond the reference, like the Detailer itself) -------------------------------------------
 * Several masked subjects that move: the per-region form labels the union over frames, where a walking person is a smear and
 * two people whose paths cross are one component; the track form has one box per frame, which spans every subject.  Here the
 * mask is labelled in space and time, a subject is a set of space-time components, and every (subject, frame) gets a window of
 * its own, all of one size.  The host (lanpaint_amd/detail_subjects.py, plan_subjects) groups components into subjects and plans
 * each subject's path.  A job reads two tables back: the components table (n and 7 ints per component, about 112 KB at the
 * cap) and the boxes table (about 83 KB at 64 subjects x 81 frames).                                                          */

/* Connected components of  S = {(f, y, x): mask[f, y, x] > 0.5}  -- no union over planes --, 26-connected in (f, y, x).  A
 * component's label is 1 + the rank of its smallest flat index (f * height + y) * width + x: labels run 1..n in raster order of
 * first voxel, 0 is background -- scipy.ndimage.label(S, ones((3, 3, 3))).
 *   mask    [frames, height, width] fp32
 *   labels  out, device, int32 [frames, height, width]; exact whatever n is
 *   table   out, device, int32 [1 + 7 * LP_DETAIL_MAX_COMPONENTS]: table[0] = n, the true count even past the cap; for
 *           id = 1 .. min(n, cap), table[1 + 7 * (id - 1) ..] = {f_min, f_max, row_min, row_max, col_min, col_max, volume},
 *           bounds inclusive; rows past n hold {frames, -1, height, -1, width, -1, 0}
 *   workspace  device, LP_COMPONENTS_FRAMES_WS_BYTES(frames, height, width) bytes, 16-byte aligned
 * lp_mask_components' seven launches on the volume (tile and border per frame) plus one that unites every frame with the one
 * before it (csrc/label_kernel.hip); integer atomics only, the result does not depend on the order of arrival.
 * LP_E_INVALID: null pointer, frames <= 0, a side outside 1..LP_DETAIL_MAX_SIDE, a short workspace; LP_E_ALIGN: workspace not
 * 16-byte aligned; LP_E_UNSUPPORTED: frames > 65535 or frames * height * width > 2^30 (parents are int32 flat indices).  All
 * checked before any HIP call.                                                                                               */
#define LP_COMPONENTS_FRAMES_WS_BYTES(frames, height, width) \
    ((((int64_t)(frames) * (height) * (width) + 1023) / 1024) * 4100)
LP_API int lp_mask_components_frames(const float* mask, int32_t frames, int32_t height, int32_t width, int32_t* labels,
                                     int32_t* table, void* workspace, int64_t workspace_bytes, void* stream);

/* One bounding box per (subject, frame) of a label volume.
 *   labels  device int32 [frames, height, width] (lp_mask_components_frames)
 *   owner   device int32 [owner_len]: owner[label] = subject + 1, 0 for a label no subject owns; a label >= owner_len and an
 *           owner outside 1..subjects are nobody's
 *   boxes   out, device, int32 [subjects, frames, 4] = {row_min, row_max, col_min, col_max}, inclusive, over the voxels of
 *           frame f whose label's owner is s + 1; {height, -1, width, -1} where there is none.  Initialised by this call.
 * One launch over every frame, integer atomics only.  LP_E_INVALID: null pointer, frames <= 0, a side outside
 * 1..LP_DETAIL_MAX_SIDE, owner_len < 1, subjects outside 1..LP_DETAIL_MAX_REGIONS; LP_E_UNSUPPORTED: frames > 65535.         */
LP_API int lp_subject_boxes(const int32_t* labels, int32_t frames, int32_t height, int32_t width, const int32_t* owner,
                            int32_t owner_len, int32_t subjects, int32_t* boxes, void* stream);

/* lp_detail_resample for a window per (subject, image):  dst [subjects * batch, out_h, out_w, channels], subject-major,
 * dst[s * batch + f] = lp_detail_resample of the window at origins[s * batch + f] of src[f], bit for bit, in one launch.
 *   origins  DEVICE int32 [subjects * batch, 2] = (y0, x0); an origin is clamped so that its window lies inside the image
 * With `labels` the source is a mask (channels == 1) and subject s sees image f with foreign components erased, as in
 * lp_detail_resample_regions but read from image f's label plane:
 *   labels  device int32 [batch, src_h, src_w] (lp_mask_components_frames), or NULL: no erasing;  owner  device int32 [owner_len]
 *   scratch device fp32 [subjects * batch * win_h * win_w], 16-byte aligned: the erased windows, needed with `labels` when the
 *           size changes
 * Errors as lp_detail_resample, plus LP_E_INVALID: subjects outside 1..LP_DETAIL_MAX_REGIONS, null origins, labels with
 * channels != 1 or without owner / scratch; LP_E_UNSUPPORTED: subjects * batch > 65535.                                      */
typedef struct lp_detail_resample_subjects_desc {
    int32_t batch, src_h, src_w, channels;
    int32_t subjects, win_h, win_w, owner_len;
    int32_t out_h, out_w, ksize_x, ksize_y;
    const int32_t* origins;
    const float*   src;
    const int32_t* bounds_x;
    const float*   weights_x;
    const int32_t* bounds_y;
    const float*   weights_y;
    float*         dst;
    const int32_t* labels;
    const int32_t* owner;
    float*         scratch;
} lp_detail_resample_subjects_desc;
LP_API int lp_detail_resample_subjects(const lp_detail_resample_subjects_desc* desc, void* stream);

/* lp_detail_stitch composed over subjects, in subject order, frame by frame:
 *   out_0 = original;   out_{s+1}[f] = lp_detail_stitch(out_s[f], detail[s * batch + f], mask_s[f], window (s, f));   out = out_subjects
 * bit for bit, mask_s[f] frame f's mask with foreign components erased as above (labels NULL: the mask itself for every
 * subject).  Windows of different subjects may overlap, so the order is part of the result.  One streaming copy original ->
 * out, then one launch per subject over the tiles of all frames' windows (the frame on a grid axis), in place on out: one
 * thread reads and writes a given element, and the mask halo is read from the mask, never from out.
 *   origins  DEVICE int32 [subjects * batch, 2] = (y0, x0), clamped as above
 *   mask     [batch, height, width]: one plane per image
 *   detail   [subjects * batch, win_h, win_w, channels], subject-major, already at the window's size
 * Errors as lp_detail_stitch, plus LP_E_INVALID: subjects outside 1..LP_DETAIL_MAX_REGIONS, null origins, labels without
 * owner.                                                                                                                    */
typedef struct lp_detail_stitch_subjects_desc {
    int32_t batch, height, width, channels;
    int32_t subjects, win_h, win_w, k;
    int32_t owner_len, reserved0;
    const int32_t* origins;
    const float*   mask;
    const float*   original;
    const float*   detail;
    float*         out;
    const int32_t* labels;
    const int32_t* owner;
} lp_detail_stitch_subjects_desc;
LP_API int lp_detail_stitch_subjects(const lp_detail_stitch_subjects_desc* desc, void* stream);

/* ---- Detailer colour match (beyond the reference, like the Detailer itself) -----------------------------------------------------
 * A crop that went through resample, VAE, sampler and VAE comes back with a small gain and offset per channel.  Outside the
 * mask the decoded crop shows what the original crop shows, so statistics taken there are like for like: three calls between
 * decode and any of the stitches measure the drift (lp_color_stats), turn it into one affine map per image and channel
 * (lp_color_fit) and undo it (lp_color_apply).  Everything stays on the device; nothing is read back.
 * Sides are 1..LP_DETAIL_MAX_SIDE, channels 1..LP_DETAIL_MAX_CHANNELS, margin 0..LP_COLOR_MAX_MARGIN.                        */
#define LP_COLOR_MIN_COUNT  64    /* lp_color_fit: a pooled window with fewer kept pixels than this fits nothing (gain 1, bias 0) */
#define LP_COLOR_MAX_MARGIN 25
#define LP_COLOR_TILE_H     32    /* lp_color_stats: one block and one partial row per tile of this many pixels                */
#define LP_COLOR_TILE_W     128
#define LP_COLOR_METHOD_MEAN     0
#define LP_COLOR_METHOD_MEAN_STD 1

/* Masked sums of two images over the pixels far enough from the mask.
 *   detail, reference  [batch, height, width, channels] fp32
 *   mask     [mask_batch, height, width] fp32, mask_batch 1 or batch; or NULL: every pixel is kept (mask_batch is not read)
 *   keep     pixel (y, x) of image i is kept when every mask element of that image with |y' - y| <= margin and |x' - x| <= margin
 *            inside the image is <= 0.5; neighbours outside the image do not count
 *   stats    out, device, fp64 [batch, 1 + 4 * channels]: row i = {n, then per channel sum d, sum r, sum d^2, sum r^2} over the
 *            kept pixels of image i.  n is an exact integer.
 *   workspace  device, LP_COLOR_WS_BYTES(batch, height, width, channels) bytes, 16-byte aligned: one partial row per tile
 * Every term is converted to fp64 first, so a square is exact, and is added in fp64 from the first add, each operation rounded
 * on its own.  Two plain launches on `stream` (csrc/color_kernel.hip): the tiles, each with the mask's halo as bits in LDS,
 * write their partial rows; the second folds an image's partial rows in a fixed order.  No floating-point atomic anywhere: the
 * result is the same bits on every run.
 * LP_E_INVALID: null pointer, batch <= 0, a side, the channel count or margin outside the limits, mask_batch, a short
 * workspace; LP_E_ALIGN: workspace not 16-byte aligned; LP_E_UNSUPPORTED: batch > 65535.  All checked before any HIP call.  */
#define LP_COLOR_WS_BYTES(batch, height, width, channels)                                                  \
    ((int64_t)(batch) * (((height) + LP_COLOR_TILE_H - 1) / LP_COLOR_TILE_H) *                             \
     (((width) + LP_COLOR_TILE_W - 1) / LP_COLOR_TILE_W) * (1 + 4 * (channels)) * 8)
typedef struct lp_color_stats_desc {
    int32_t batch, height, width, channels;
    int32_t mask_batch, margin;
    const float* detail;
    const float* reference;
    const float* mask;
    double*      stats;
    void*        workspace;
    int64_t      workspace_bytes;
} lp_color_stats_desc;
LP_API int lp_color_stats(const lp_color_stats_desc* desc, void* stream);

/* stats [batch, 1 + 4 * channels] -> coef, device, fp32 [batch, channels, 2] = (gain, bias).  One launch, fp64, every operation
 * rounded on its own.  With L = clip_frames (0: L = batch; L must divide batch), k = smooth (0, or odd 1..129), s = strength:
 *   pool      image i is frame f = i % L of clip q = i / L.  P = the sum, in ascending frame order, of the stats rows of frames
 *             max(0, f - k / 2) .. min(L - 1, f + k / 2) of clip q (k = 0: of the whole clip).  The window is cut at the clip's
 *             ends, not clamped: no frame is counted twice.
 *   guard     N = P.n < LP_COLOR_MIN_COUNT: gain = 1, bias = 0
 *   moments   per channel  md = P.d / N, mr = P.r / N, vd = P.dd / N - md * md, vr = P.rr / N - mr * mr
 *   gain      LP_COLOR_METHOD_MEAN: g = 1.  LP_COLOR_METHOD_MEAN_STD: g = 1 when vd <= 1e-8 or vr is not >= 0, otherwise
 *             g = sqrt(vr / vd) limited to [0.25, 4]
 *   bias      b = mr - g * md
 *   strength  gain = 1 + s * (g - 1), bias = s * b  (lerp(detail, matched, s)), both then rounded to fp32
 * LP_E_INVALID: null pointer, batch <= 0, channels outside the limits, clip_frames < 0 or not a divisor of batch, smooth even
 * (other than 0) or outside 0..129, an unknown method, strength outside [0, 1]; LP_E_UNSUPPORTED: batch > 65535.             */
typedef struct lp_color_fit_desc {
    int32_t batch, channels;
    int32_t clip_frames, smooth;
    int32_t method, reserved0;
    double  strength;
    const double* stats;
    float*        coef;
} lp_color_fit_desc;
LP_API int lp_color_fit(const lp_color_fit_desc* desc, void* stream);

/* out[i, y, x, c] = fadd_rn(fmul_rn(detail[i, y, x, c], coef[i, c, 0]), coef[i, c, 1]), unfused.  One launch, 16 bytes per lane
 * when detail, out and every image's first element are 16-byte aligned.  out may be detail.
 *   detail, out  [batch, height, width, channels] fp32;  coef  [batch, channels, 2] fp32 (lp_color_fit)
 * LP_E_INVALID: null pointer, batch <= 0, a side or the channel count outside the limits; LP_E_UNSUPPORTED: batch > 65535.  */
typedef struct lp_color_apply_desc {
    int32_t batch, height, width, channels;
    const float* detail;
    const float* coef;
    float*       out;
} lp_color_apply_desc;
LP_API int lp_color_apply(const lp_color_apply_desc* desc, void* stream);

/* ---- Masked-area fill and outpaint canvas (beyond the reference) ------------------------------------------------------------------
 * The sampler ignores the latent under the mask, the VAE encoder does not ignore the pixels there: its receptive field reaches
 * across the mask's edge.  lp_mask_fill replaces the masked pixels by a smooth continuation of the known ones before the
 * encode; lp_outpaint_pad builds the extended canvas and its mask.  Everything stays on the device; nothing is read back.
 * Sides are 1..LP_DETAIL_MAX_SIDE, channels 1..LP_DETAIL_MAX_CHANNELS.                                                       */
#define LP_FILL_TILE 32    /* lp_mask_fill: the side of the tile of a level one block stages                                   */
#define LP_FILL_SPAN 5     /*               the levels above that tile one launch covers                                       */

/* Push-pull pyramid fill, every image on its own, fp32, every operation rounded on its own.
 *   image, out  [batch, height, width, channels] fp32, out != image
 *   mask        [mask_batch, height, width] fp32, mask_batch 1 or batch.  A pixel is masked when mask > 0.5 (a NaN is not), else
 *               known, as for lp_mask_bbox
 *   ws          device, lp_fill_ws_bytes(batch, height, width, channels) bytes, 16-byte aligned; contents need not be set
 * levels  (h_0, w_0) = (height, width), (h_{l+1}, w_{l+1}) = (ceil(h_l / 2), ceil(w_l / 2)) down to (1, 1): levels 0 .. L - 1
 * pull    k_0 = known, v_0 = image where known (never read elsewhere).  For l = 0 .. L - 2 and coarse pixel (i, j): the children
 *         (2 i + dy, 2 j + dx) in the order (0,0), (0,1), (1,0), (1,1) that lie inside level l and have k_l = 1 are present,
 *         n = their number, k_{l+1} = (n > 0), and per channel s = 0, s = s + v_l(child) for each present child in that order,
 *         v_{l+1} = s / (float)n (IEEE)
 * empty   k_{L-1} = 0: the image has no known pixel; out = image, bit for bit
 * push    f_{L-1} = v_{L-1}; for l = L - 2 .. 0: f_l = v_l where k_l = 1, elsewhere the 2x bilinear upsample of f_{l+1} with
 *         pixel centres aligned and taps clamped.  Per axis, fine index i over a coarse axis of n' entries: i even: i0 = i / 2 - 1,
 *         weights (0.25, 0.75); i odd: i0 = (i - 1) / 2, weights (0.75, 0.25); taps t0 = clamp(i0, 0, n' - 1),
 *         t1 = clamp(i0 + 1, 0, n' - 1).  Rows first, r(x') = a0 * f(ty0, x') + a1 * f(ty1, x') for both column taps, then
 *         up = b0 * r(tx0) + b1 * r(tx1); every product and every sum rounded.
 * out     a known pixel takes the image's value bit for bit, a masked one f_0.  No output depends on the image under the mask.
 * The whole job is enqueued on `stream` by this call (csrc/fill_kernel.hip): one launch covers LP_FILL_SPAN levels, so a
 * 720 x 1280 image (12 levels) takes three launches each way.  The same bits on every run.
 * LP_E_INVALID: null pointer, batch <= 0, a side or the channel count outside the limits, mask_batch, out == image, a short
 * workspace; LP_E_ALIGN: ws not 16-byte aligned; LP_E_UNSUPPORTED: batch > 65535.  All checked before any HIP call.           */
typedef struct lp_fill_desc {
    int32_t batch, height, width, channels;
    int32_t mask_batch, reserved0;
    const float* image;
    const float* mask;
    float*       out;
    void*        ws;
    int64_t      ws_bytes;
} lp_fill_desc;
LP_API int lp_mask_fill(const lp_fill_desc* desc, void* stream);

/* Bytes of lp_mask_fill's workspace: per image and pixel of levels 1 .. L - 1, `channels` fp32 values and one flag byte, the
 * total rounded up to 16 (and at least 16).  Host arithmetic, no HIP call.  A negative LP_E_* for arguments lp_mask_fill
 * refuses.                                                                                                                   */
LP_API int64_t lp_fill_ws_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels);

/* ---- lp_mask_fill, the patch form: reserved0 = LP_FILL_PATCH(r, levels, iters, seed) ------------------------------------------------
 * reserved0 == 0 is the push-pull fill above, unchanged.  The patch form first makes that fill and then replaces it, under the
 * mask, by texture copied from the known part of the same image (a PatchMatch search and vote over a pyramid of 8-bit codes).
 * Every image on its own; integers throughout except the pre-fill and the final division; the same bits on every run and for
 * every split of a batch.  (csrc/patch_fill_kernel.hip.)
 *
 * Mode word: bit 0 = 1; bits 4..7 r, the patch radius (P = 2 r + 1), 1..LP_FILL_PATCH_MAX_RADIUS; bits 8..11 levels,
 * 1..LP_FILL_PATCH_MAX_LEVELS; bits 12..15 iters, 1..LP_FILL_PATCH_MAX_ITERS; bits 16..31 seed, 0..65535; bits 1..3 zero.
 * LP_E_INVALID: bit 0 clear with another bit set, bits 1..3, a field outside its range, ws_bytes below
 * LP_FILL_PATCH_WS_BYTES(...);  LP_E_UNSUPPORTED: channels > LP_FILL_PATCH_MAX_CHANNELS.  All checked before any HIP call,
 * next to the checks above.
 *
 * 1 codes    pp = the push-pull result (the rule above; `out` holds it first).  code(v) = clamp(floor(fl(fl(v * 255) + 0.5)), 0, 255)
 *            in fp32, a NaN gives 0.  I_0 = code(pp) per channel, so a known pixel holds its own code; hole_0 = mask > 0.5 (a NaN
 *            is not).  A pixel's codes are one 32-bit word, channel c in byte c, unused bytes 0.
 * 2 pyramid  levels 0 .. levels - 1, (h_{l+1}, w_{l+1}) = (ceil(h_l / 2), ceil(w_l / 2)).  Per channel I_{l+1}(i, j) =
 *            (sum + n / 2) / n (integer division) over the children (2 i + dy, 2 j + dx), dy, dx in {0, 1}, that lie inside level
 *            l, n = their number (1, 2 or 4); hole_{l+1} = the OR of those children's hole_l.
 * 3 sets     per level: p is a TARGET when a pixel p + d, d in [-r, r]^2, inside the picture is a hole (the hole dilated by r,
 *            Chebyshev); s is a SOURCE when all of s + [-r, r]^2 lies inside the picture and none of it is a hole.  The field
 *            NNF holds per target a source centre or INVALID.
 * 4 distance T is the working image: I_l with the hole pixels at their current estimate.  D(p, s) = the sum over d in [-r, r]^2
 *            with p + d inside the picture, and over the channels, of |T(p + d) - I_l(s + d)|.  A candidate must be a source;
 *            candidates are ordered by the key (D, s_y, s_x) and the lowest key wins.
 * 5 search   one round reads NNF_in and writes NNF_out for every target p (no order between pixels).  Candidates, in this order:
 *            (a) NNF_in(p) if valid;  (b) for step in (1, 4) and e in ((0, -1), (-1, 0), (0, 1), (1, 0)) (e = (e_y, e_x)):
 *            n = p + step * e; if n is inside the picture, a target and NNF_in(n) valid: NNF_in(n) - step * e;  (c) for
 *            j = 0, 1, ... while R_j = max(h_l, w_l) >> j >= 1: centre + (u_y, u_x), centre = the best so far (p itself while
 *            none is valid), u = (int)((word * (2 R_j + 1)) >> 32) - R_j with the product in 64 bits, word = word 0 for u_y and
 *            word 1 for u_x of Philox4x32-10 (Random123) with counter (p_y * 65536 + p_x [64 bit], (level << 40 | round << 32 |
 *            j) [64 bit]) and key `seed` [64 bit]; the best is updated after every j.  `round` counts the rounds of a level from
 *            0.  A candidate outside the picture or no source is dropped.  NNF_out(p) = the best, INVALID while there is none.
 *            Neither the counter nor the key holds the image's index.
 * 6 vote     each hole pixel q, per channel: sum = the sum of I_l(NNF(p) + d) over d in [-r, r]^2 with p = q - d inside the
 *            picture and NNF(p) valid, n = the number of such d; n > 0: T(q) = (sum + n / 2) / n; n = 0: T(q) stays.
 * 7 schedule coarsest level: T = I_l, NNF all INVALID, then iters x (search, vote).  From level l + 1 to l: T = I_l, NNF_l(p) =
 *            2 NNF_{l+1}(p >> 1) + (p & 1) (per coordinate) for a target p whose NNF_{l+1}(p >> 1) is valid, kept when it lies
 *            inside level l and is a source of level l, else INVALID; then one vote, then iters x (search, vote).
 * 8 out      a known pixel: the image's bits.  A hole pixel with n > 0 in the last vote of level 0: (float)code / 255.0f (IEEE
 *            division) per channel.  A hole pixel with n = 0 there: pp.
 * So an image with no hole comes back bit for bit, an image with no source is the push-pull result bit for bit, and no output
 * depends on the image under the mask.
 *
 * Workspace: LP_FILL_PATCH_WS_BYTES(lp_fill_ws_bytes(batch, height, width, channels), batch, height, width, levels) bytes.  First
 * the push-pull form's part, lp_fill_ws_bytes(...) bytes (a multiple of 16); then for level l = 0 .. levels - 1, with
 * n_l = batch * h_l * w_l and each plane's bytes rounded up to 16, image b at element b * h_l * w_l of a plane, in this order:
 *   codes  n_l uint32   I_l                          work   n_l uint32   T
 *   nnf    n_l int32    the field a level ends with and the vote reads: s_y * 65536 + s_x, INVALID = -1 (also where p is no target)
 *   nnf2   n_l int32    the other field of the rounds
 *   hole   n_l uint8    hole_l                       sets   n_l uint8    bit 0 hole, bit 1 target, bit 2 source
 * LP_FILL_PATCH_LEVEL_BYTES(n) is one level's share.  Contents need not be set: no byte is read before it is written.
 * Launches on `stream`: the push-pull form's, then 2 * levels for codes, pyramid and sets, and per level one field launch and
 * iters x (search, vote), one more vote below the coarsest level.  A search or vote block is a 16 x 16 tile (LP_FILL_PATCH_TILE)
 * with its r-halo in LDS; a tile without target (search) or hole (vote) leaves after its flags.                                   */
#define LP_FILL_PATCH_MAX_RADIUS   4
#define LP_FILL_PATCH_MAX_LEVELS   6
#define LP_FILL_PATCH_MAX_ITERS    8
#define LP_FILL_PATCH_MAX_CHANNELS 4
#define LP_FILL_PATCH_TILE         16
#define LP_FILL_PATCH(r, levels, iters, seed)                                                                              \
    ((int32_t)(1u | ((uint32_t)(r) << 4) | ((uint32_t)(levels) << 8) | ((uint32_t)(iters) << 12) | ((uint32_t)(seed) << 16)))
#define LP_FILL_PATCH_LEVEL_BYTES(n) (4 * (((int64_t)(n) * 4 + 15) / 16 * 16) + 2 * (((int64_t)(n) + 15) / 16 * 16))
/* `pull_bytes` = lp_fill_ws_bytes(batch, height, width, channels); h_l = ((height - 1) >> l) + 1, the side halved l times, rounded up */
#define LP_FILL_PATCH_SIDE(s, l) ((((int64_t)(s) - 1) >> (l)) + 1)
#define LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, l)                                                            \
    ((l) < (levels) ? LP_FILL_PATCH_LEVEL_BYTES((int64_t)(batch) * LP_FILL_PATCH_SIDE(height, l) * LP_FILL_PATCH_SIDE(width, l)) : 0)
#define LP_FILL_PATCH_WS_BYTES(pull_bytes, batch, height, width, levels)                                                   \
    ((int64_t)(pull_bytes) + LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, 0) +                                     \
     LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, 1) + LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, 2) +   \
     LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, 3) + LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, 4) +   \
     LP_FILL_PATCH_WS_LEVEL(batch, height, width, levels, 5))

/* The outpaint canvas and its mask, one launch.  H' = top + height + bottom, W' = left + width + right.
 *   image      [batch, height, width, channels] fp32
 *   mask       [mask_batch, height, width] fp32, mask_batch 1 or batch; mask_batch 0: no mask (the pointer is not read)
 *   image_out  [batch, H', W', channels]: the original inside its rectangle, bit for bit, 0.0 elsewhere
 *   mask_out   [max(mask_batch, 1), H', W']: max(band, m).  band = 1.0 outside the original's rectangle and inside it within
 *              `overlap` pixels of a side whose pad is positive, 0.0 elsewhere (hard, not feathered); m = the incoming mask's
 *              value, soft values kept, 0 outside the rectangle or without a mask; a NaN m gives band
 * LP_E_INVALID: null pointer, batch <= 0, a side or the channel count outside the limits, mask_batch not 0, 1 or batch, a
 * negative pad or overlap, all four pads 0, a canvas side above LP_DETAIL_MAX_SIDE; LP_E_UNSUPPORTED: batch > 65535.         */
typedef struct lp_outpaint_desc {
    int32_t batch, height, width, channels;
    int32_t mask_batch, left, top, right;
    int32_t bottom, overlap, reserved0;
    const float* image;
    const float* mask;
    float*       image_out;
    float*       mask_out;
} lp_outpaint_desc;
LP_API int lp_outpaint_pad(const lp_outpaint_desc* desc, void* stream);

/* ---- Multiband blend (beyond the reference) -------------------------------------------------------------------------------------
 * Every path that puts a generated image back into the original ends in lp_mask_blend's rule: one feather of at most 51 pixels.
 * What low-frequency difference a VAE round trip, an outpaint continuation or a detailed crop leaves is squeezed into that one
 * band.  lp_multiband_blend is the Burt-Adelson blend: every frequency band is blended over a width in proportion to its
 * wavelength.  It goes after any stitch or decode (stitch hard, blend_overlap = 1, then blend original and stitched through
 * the mask).  Everything stays on the device; nothing is read back.
 *   image1 (a), image2 (b), out  [batch, height, width, channels] fp32, finite; out != image1, out != image2
 *   mask                         [mask_batch, height, width] fp32, mask_batch 1 or batch
 *   levels                       >= 0
 *   ws                           device, lp_multiband_ws_bytes(batch, height, width, channels, levels) bytes, 16-byte aligned;
 *                                contents need not be set
 * Every image of the batch is independent of the others.  Every product, sum and difference below is one fp32 operation
 * rounded on its own; nothing is fused.
 * levels    (h_0, w_0) = (height, width), (h_{l+1}, w_{l+1}) = (ceil(h_l / 2), ceil(w_l / 2)).  The level count n is the smaller
 *           of `levels` and the number of halvings until (1, 1); a 1 x 1 image has n = 0.
 * weight    W_0 = (m > 0) ? min(m, 1) : 0; a NaN mask value gives 0.  The soft mask is used as given: no binarisation, no
 *           dilation.
 * diff      D_0 = b - a.
 * REDUCE    level l -> l + 1, separable, axis 0 (rows) first over the full width, then axis 1.  Along an axis of length N,
 *           output i reads inputs 2 i - 2 .. 2 i + 2, each index clamped to [0, N - 1]:
 *           s = 0.0625 * v[-2]; s = s + 0.25 * v[-1]; s = s + 0.375 * v[0]; s = s + 0.25 * v[+1]; s = s + 0.0625 * v[+2],
 *           in that order.  D_{l+1} = REDUCE(D_l) and W_{l+1} = REDUCE(W_l) for l < n.
 * EXPAND    level l + 1 -> the size of level l, axis 0 first (giving [h_l, w_{l+1}]), then axis 1.  Along an axis, output i has
 *           p = i / 2 (rounded down), coarse indices clamped to the coarse length.  i even: e = 0.125 * c[p - 1];
 *           e = e + 0.75 * c[p]; e = e + 0.125 * c[p + 1].  i odd: 0.5 * c[p] + 0.5 * c[p + 1].
 * collapse  R_n = W_n * D_n.  For l = n - 1 .. 0: Lap_l = D_l - EXPAND(D_{l+1}), R_l = EXPAND(R_{l+1}) + W_l * Lap_l (the
 *           product first, then the sum with the expansion on the left).  out = a + R_0.  levels = 0 is a + W_0 * (b - a).
 * What follows from the rule: image1 == image2 gives image1 bit for bit whatever the mask; an all-zero mask gives image1 bit
 * for bit (inputs that are not -0); a pixel whose Chebyshev distance to every pixel with W_0 > 0 exceeds 2^(n+2) - 4 is image1
 * bit for bit (REDUCE carries weight out by 2 * 2^l per level, EXPAND by 2^l): levels = 5 touches nothing further than 124
 * pixels from the mask.
 * The whole job is enqueued on `stream` by this call (csrc/multiband_kernel.hip): n reduce launches and max(n, 1) collapse
 * launches.  Level 0 is never stored, R_n is formed where it is read.  The same bits on every run.
 * LP_E_INVALID: null pointer, batch <= 0, a side or the channel count outside the limits (1..LP_DETAIL_MAX_SIDE,
 * 1..LP_DETAIL_MAX_CHANNELS), mask_batch, levels < 0, out == image1 or image2, a short workspace; LP_E_ALIGN: ws not 16-byte
 * aligned; LP_E_UNSUPPORTED: batch > 65535.  All checked before any HIP call.                                                 */
typedef struct lp_multiband_desc {
    int32_t batch, height, width, channels;
    int32_t mask_batch, levels;
    const float* image1;
    const float* image2;
    const float* mask;
    float*       out;
    void*        ws;
    int64_t      ws_bytes;
} lp_multiband_desc;
LP_API int lp_multiband_blend(const lp_multiband_desc* desc, void* stream);

/* Bytes of lp_multiband_blend's workspace: batch * sum over l = 1 .. n of h_l * w_l * (2 * channels + 1) * 4 -- per image and
 * pixel of levels 1 .. n, D with `channels` floats, W with one and R with `channels` -- rounded up to 16 (and at least 16).
 * Host arithmetic, no HIP call.  A negative LP_E_* for arguments lp_multiband_blend refuses.                                */
LP_API int64_t lp_multiband_ws_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels, int32_t levels);

/* ---- lp_multiband_blend, the focus form: levels = LP_MULTIBAND_FOCUS(edge, ring, strength16, per_frame) -------------------------------
 * Every levels >= 0 is the blend above, unchanged.  A negative `levels` is a mode word; the only form it names is focus match: measure
 * how soft the edges of the footage around the mask are, measure how soft the edges under the mask are, and blur the masked area
 * by the difference.  What a decoder returns under the mask is as sharp as the model draws; the footage around it is as soft as the
 * lens, the motion, the codec or an upscale left it.  The form goes behind the stitch or decode (and the temporal smooth) and in
 * front of the multiband blend and the grain match -- blur removes grain, so grain goes back after it.  (csrc/focus_kernel.hip.)
 *   image1   the picture to correct (the stitched or decoded result); image2 where the reference sharpness is read: the same
 *            tensor or the untouched original, same shape.  image1 == image2 is allowed; out != image1 and out != image2 stay.
 * Mode word: bit 31 set; bits 0..7 edge, 1..255 grey levels; bits 8..11 ring, 1..LP_FOCUS_MAX_RING tiles; bits 12..16 strength16,
 * 0..16 sixteenths; bit 17 per_frame; bits 18..30 zero (so levels = -1 stays LP_E_INVALID).  LP_E_INVALID: a field outside its range,
 * a bit of 18..30, and everything the plain form refuses, in its order (LP_E_ALIGN is answered before a short workspace);
 * LP_E_UNSUPPORTED: batch > 65535, or per_frame = 0 with batch * height * width > 2^30 (the pooled sums stay inside 64 bits).  All
 * before any HIP call.  lp_multiband_ws_bytes(batch, height, width, channels, word) returns LP_FOCUS_WS_BYTES(...) or those codes.
 *
 * The rule.  Integers up to the fit; the fit in fp64 with + - * / only, each rounded on its own; the blur in fp32 with every product
 * and sum rounded on its own.  No exp, log or pow.  The same bits on every run, for every tiling and every split of a batch
 * (per_frame = 1; the pooled form measures the whole batch it is given).
 * codes    code(v) = (int)(fl(fl(t * 255) + 0.5)) in fp32, t = v clamped to 0..1, a NaN gives 0.  Y = (77 c0 + 150 c1 + 29 c2 + 128)
 *          >> 8 of the codes of a pixel's first three channels; with fewer than three channels Y = c0.
 * scales   A = Y through the separable binomial (1, 2, 1) (variance 0.5), B = Y through the separable binomial
 *          (1, 8, 28, 56, 70, 56, 28, 8, 1) (variance 2), unnormalised exact integers: A carries a factor 16, B a factor 65536.
 *          A pixel takes part only if its whole 11 x 11 support (Chebyshev distance 5) lies inside the image.  Central
 *          differences: gx = P(y, x + 1) - P(y, x - 1), gy = P(y + 1, x) - P(y - 1, x), gA^2 = gx^2 + gy^2 on A, gB^2 on B, int64.
 *          An EDGE pixel has gB^2 >= (edge * 2 * 65536)^2 = (edge * 131072)^2.
 * regions  masked(p) = mask(p) > 0.5 (a NaN is not masked).  Tiles are 32 x 32 from the origin (LP_FOCUS_TILE); a tile is MARKED
 *          when it holds a masked pixel.  INSIDE: all 121 pixels of the support are masked; read on image1.  RING: none of the 121
 *          is masked, and the pixel's tile lies within `ring` tiles (Chebyshev, in tiles) of a marked tile; read on image2.
 * stats    per image and region, over the region's edge pixels: n, SA = sum of gA^2, SB = sum of floor(gB^2 / 65536) (the shift
 *          keeps SB of a 32768 x 32768 image inside an int64), all int64.  Integer sums: any order gives the same bits.
 * fit      per image (per_frame = 1) or on the sums over the batch.  A side with n < LP_FOCUS_MIN_COUNT fits nothing: K = 0, and
 *          that side's variance is reported as LP_FOCUS_NO_FIT.  Else a = (double)SA / 256, b = (double)SB / 65536, r = a / b,
 *          q = r * r (the squared ratio of the mean squared gradients (SA / 16^2) / (SB' / 65536^2), SB' the unshifted sum);
 *          var = (2 - 0.5 * q) / (q - 1) for q > 1, LP_FOCUS_MAX_VAR for q <= 1 (a step edge of variance s^2 has
 *          q = (s^2 + 2) / (s^2 + 0.5)).  d = var_ring - var_inside, 0 if that is not positive; v = (strength16 / 16) * d, limited to
 *          LP_FOCUS_MAX_VAR (16 px^2, sigma 4); K = (int)(v * 32 + 0.5): the variance to add in thirty-seconds of a px^2.
 * kernel   k = K >> 4, t = K & 15.  b_k(i) = C(2 k, k + i) / 4^k, the binomial of order 2 k and variance k / 2 exactly: the integer
 *          coefficient (< 2^64 up to order 66) converted to fp64, round to nearest even, times the exact power of two; 0 for
 *          |i| > k.  w(i) = (float)(((16 - t) * b_k(i) + t * b_{k+1}(i)) / 16) for |i| <= 33.  A mixture of zero-mean kernels has
 *          the mixed variance, so w has variance K / 32 before the rounding to fp32.
 * apply    separable, rows first (along x into a plane of the workspace), then columns.  r = k + 1 for t > 0, else k.  Along an
 *          axis: s = w(-r) * v[-r]; s = s + w(i) * v[i] for i = -r + 1 .. r in that order, coordinates clamped to the image.
 *          m = (mask > 0) ? min(mask, 1) : 0 (a NaN gives 0); out = image1 + m * (blur - image1), the difference, the product and
 *          the sum in that order.  Where m == 0 or K == 0, out holds image1's bits.  A tile without m > 0 only copies; the rows pass
 *          skips a tile no column pass reads.
 * What follows: an all-zero mask gives image1 bit for bit; a masked area as soft as or softer than its surroundings gives image1
 * bit for bit; so does an image with a side under 11 pixels; nothing further than 33 pixels from a pixel with m > 0 changes.
 * NOT handled: sharpening (a generated side softer than the ring is left alone); focus that varies across the mask (one variance
 * per frame or per clip); textures without edges (they fall under LP_FOCUS_MIN_COUNT and nothing happens).
 *
 * Workspace, LP_FOCUS_WS_BYTES(batch, height, width, channels) bytes, contents need not be set (no byte is read before it is
 * written), at the offsets of the macros below, each a multiple of 16:
 *   FLAGS  uint8 [batch][ceil(height / 32)][ceil(width / 32)], rows of mask_batch images used: bit 0 a masked pixel, bit 1 m > 0
 *   STATS  int64 [batch][2][3]: region 0 ring, 1 inside; {n, SA, SB}
 *   VAR    fp64  [batch][2]: var_ring, var_inside as fitted (pooled: the same pair in every row)
 *   K      int32 [batch]                       TAPS   fp32 [batch][LP_FOCUS_TAPS]: w(i) at index 33 + i
 *   PLANE  fp32  [batch][height][width][channels]: the rows pass
 * Five launches on `stream`: flags (it also clears STATS), stats, fit (one block), rows, columns.  The blur is two launches through
 * PLANE, not one launch with a 33-pixel halo in LDS: at four channels that tile is 98 x 98 x 16 bytes = 150 KB of the 160 KB a CU
 * has, one block a CU.                                                                                                          */
#define LP_FOCUS_MAX_RING  8
#define LP_FOCUS_MIN_COUNT 64
#define LP_FOCUS_MAX_VAR   16
#define LP_FOCUS_NO_FIT    (-1.0)
#define LP_FOCUS_TILE      32
#define LP_FOCUS_TAPS      67
#define LP_MULTIBAND_FOCUS(edge, ring, strength16, per_frame)                                                               \
    ((int32_t)(0x80000000u | (uint32_t)(edge) | ((uint32_t)(ring) << 8) | ((uint32_t)(strength16) << 12) | ((uint32_t)(per_frame) << 17)))
#define LP_FOCUS_R16(n) (((int64_t)(n) + 15) / 16 * 16)
#define LP_FOCUS_TILES(s) (((int64_t)(s) + LP_FOCUS_TILE - 1) / LP_FOCUS_TILE)
#define LP_FOCUS_WS_FLAGS(batch, height, width, channels) ((int64_t)0)
#define LP_FOCUS_WS_STATS(batch, height, width, channels) LP_FOCUS_R16((int64_t)(batch) * LP_FOCUS_TILES(height) * LP_FOCUS_TILES(width))
#define LP_FOCUS_WS_VAR(batch, height, width, channels) (LP_FOCUS_WS_STATS(batch, height, width, channels) + (int64_t)(batch) * 48)
#define LP_FOCUS_WS_K(batch, height, width, channels) (LP_FOCUS_WS_VAR(batch, height, width, channels) + (int64_t)(batch) * 16)
#define LP_FOCUS_WS_TAPS(batch, height, width, channels) (LP_FOCUS_WS_K(batch, height, width, channels) + LP_FOCUS_R16((int64_t)(batch) * 4))
#define LP_FOCUS_WS_PLANE(batch, height, width, channels)                                                                   \
    (LP_FOCUS_WS_TAPS(batch, height, width, channels) + LP_FOCUS_R16((int64_t)(batch) * LP_FOCUS_TAPS * 4))
#define LP_FOCUS_WS_BYTES(batch, height, width, channels)                                                                   \
    (LP_FOCUS_WS_PLANE(batch, height, width, channels) + LP_FOCUS_R16((int64_t)(batch) * (height) * (width) * (channels) * 4))

/* ---- Mask refine (beyond the reference) ---------------------------------------------------------------------------------------
 * Every node after the sampler takes the mask as given, and the mask is what nobody helps the user with: a painted blob, or the
 * SDF morph of two blobs, follows the subject's centroid and not its outline.  lp_mask_refine is the colour guided filter (He,
 * Sun, Tang 2013) with the image as the guide: it pulls the mask's edge onto the nearest edge of the image underneath.  It goes
 * in front of the encode, a Detailer crop, the mask fill and the multiband blend, and behind the video mask editor (every frame
 * with that frame as its guide).  Everything stays on the device; nothing is read back.
 *   guide   [batch, height, width, channels] fp32; channels 1 is a grey guide (one guide plane, a 1 x 1 system), channels >= 3
 *           uses the first three, channels 2 is refused
 *   mask    [mask_batch, height, width] fp32, mask_batch 1 or batch
 *   out     [batch, height, width] fp32; out != guide, out != mask
 *   radius  r in 1..LP_REFINE_MAX_RADIUS;  eps in [1e-6, 1], in units of the [0, 1] image scale, squared
 *   ws      device, lp_refine_ws_bytes(batch, height, width, channels, radius) bytes, 16-byte aligned; contents need not be set
 * Every image of the batch is independent of the others.
 * codes     For a guide or mask value v: t = (v > 0) ? min(v, 1) : 0 (a NaN gives 0); code = (int)(t * 255.0f + 0.5f), the fp32
 *           product and the fp32 sum each rounded on its own (no FMA), then truncated.  G_c are the guide's codes (c = 0, 1, 2;
 *           a grey guide has G_0 only), P the mask's.
 * stage 1   The window of pixel (y, x) is the (2r + 1)-square around it cut at the image border (not clamped, not reflected),
 *           n its pixel count.  S_c = sum G_c, S_p = sum P, S_cp = sum G_c * P, S_cd = sum G_c * G_d for c <= d, over the
 *           window: exact integers, at most 129^2 * 255^2 = 1 082 081 025 < 2^31, so the order of summation is free.
 * stage 2   Per pixel, in fp64, every operation rounded on its own, a product always before the sum or difference it goes
 *           into, sums from left to right:
 *             C_c  = n * S_cp - S_c * S_p,  V_cd = n * S_cd - S_c * S_d      (exact integers below 2^53)
 *             R    = (n * n) * (eps * 65025.0)
 *             m00 = V_00 + R, m11 = V_11 + R, m22 = V_22 + R, m01 = V_01, m02 = V_02, m12 = V_12
 *             c00 = m11 * m22 - m12 * m12   c01 = m02 * m12 - m01 * m22   c02 = m01 * m12 - m02 * m11
 *             c11 = m00 * m22 - m02 * m02   c12 = m01 * m02 - m00 * m12   c22 = m00 * m11 - m01 * m01
 *             det = (m00 * c00 + m01 * c01) + m02 * c02
 *             a_0 = ((c00 * C_0 + c01 * C_1) + c02 * C_2) / det
 *             a_1 = ((c01 * C_0 + c11 * C_1) + c12 * C_2) / det
 *             a_2 = ((c02 * C_0 + c12 * C_1) + c22 * C_2) / det
 *             if det is not > 0: a_0 = a_1 = a_2 = 0
 *             b   = (S_p - ((a_0 * S_0 + a_1 * S_1) + a_2 * S_2)) / n
 *           A grey guide: det = m00, a_0 = C_0 / det (0 if det is not > 0), b = (S_p - a_0 * S_0) / n.
 *           a_c and b are then rounded to fp32: the workspace holds (a_0, a_1, a_2, b) per pixel, 16 bytes (a grey guide leaves
 *           a_1 = a_2 = 0).
 * stage 3   A_c and B are the sums of a_c and b over the same window, in fp64: first the sum over the window's columns in
 *           ascending x for every row of the window, starting from +0.0, then the sum of those row sums in ascending y, starting
 *           from +0.0.  Terms outside the image are skipped (adding +0.0 for them gives the same bits).  Then
 *             t = A_0 * G_0; t = t + A_1 * G_1; t = t + A_2 * G_2; t = t + B; t = t / n; t = t / 255.0
 *           (a grey guide: t = A_0 * G_0; t = t + B; ...), and out = (float)min(max(t, 0), 1).
 * What follows from the rule: an all-zero mask gives exactly 0 and an all-one mask exactly 1.0 whatever the guide; a pixel whose
 * Chebyshev distance to every pixel with P > 0 exceeds 2r is exactly 0, and exactly 1.0 when it is that far from every pixel
 * with P < 255; a constant guide gives the mask box-blurred twice.  The same bits on every run.
 * The whole job is enqueued on `stream` by this call (csrc/refine_kernel.hip): two launches, one for stages 1 and 2 and one for
 * stage 3.  No floating-point atomics.
 * LP_E_INVALID: null pointer, batch <= 0, a side outside 1..LP_DETAIL_MAX_SIDE, channels 2, < 1 or > LP_DETAIL_MAX_CHANNELS,
 * radius outside 1..LP_REFINE_MAX_RADIUS, eps outside [1e-6, 1] or NaN, mask_batch, out == guide or mask, a short workspace;
 * LP_E_ALIGN: ws not 16-byte aligned; LP_E_UNSUPPORTED: batch > 65535.  All checked before any HIP call.                      */
#define LP_REFINE_MAX_RADIUS 64
typedef struct lp_refine_desc {
    int32_t batch, height, width, channels;
    int32_t mask_batch, radius;
    double       eps;
    const float* guide;
    const float* mask;
    float*       out;
    void*        ws;
    int64_t      ws_bytes;
} lp_refine_desc;
LP_API int lp_mask_refine(const lp_refine_desc* desc, void* stream);

/* Bytes of lp_mask_refine's workspace: batch * height * width * 16 -- (a_0, a_1, a_2, b) as fp32 per pixel.  Host arithmetic,
 * no HIP call.  A negative LP_E_* for arguments lp_mask_refine refuses.                                                       */
LP_API int64_t lp_refine_ws_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels, int32_t radius);

/* ---- Video mask stabilize (beyond the reference) --------------------------------------------------------------------------------
 * A per-frame mask that comes from a segmenter, or was painted frame by frame, flickers: its edge jitters by a pixel or two from
 * frame to frame, and single frames come back empty or carry a stray blob.  Everything downstream inherits that.  lp_mask_stabilize
 * filters the mask's signed distance field along time: a temporal median removes what lasts at most median_radius frames, a
 * binomial smoothing calms the edge.  It goes behind a per-frame segmenter or the video mask editor and in front of the mask
 * refine, the encode and the Detailer crops.  Everything stays on the device; nothing is read back.
 *   mask    [frames, height, width] fp32, binarised as lp_vmask_edt does: foreground = (v >= 0.5), a NaN is background
 *   sides   1..LP_VMASK_MAX_SIDE; frames >= 1
 * stage 1   (lp_mask_signed_d2)  q[t, y, x], int32, from the two planes lp_vmask_edt wrote for frame t: on a foreground pixel
 *           (d2_fg == 0) q = +d2_bg >= 1, on a background pixel q = -d2_fg <= -1.  Where the wanted plane holds LP_VMASK_D2_NONE
 *           q = +LP_STAB_Q_FAR (a full frame) or -LP_STAB_Q_FAR (an empty frame); 2^30 lies above every real squared distance
 *           (at most 2 * 16383^2).
 * stage 2   Temporal median, radius Tm = median_radius in 0..LP_STAB_MAX_MEDIAN: qm[t] is the median of the 2 Tm + 1 values
 *           q[clamp(t + k, 0, frames - 1)], k = -Tm..Tm.  The end frames are replicated, so the count is odd; integers, exact.
 * stage 3   s[t] = sign(qm) * sqrt((double)|qm|), the correctly rounded fp64 square root lp_vmask_edt's sdf uses, then
 *           s = min(max(s, -LP_STAB_SD_CAP), LP_STAB_SD_CAP): far from every edge, and on empty and full frames, a distance must
 *           not outweigh the frames that do have an edge nearby.
 * stage 4   Temporal smoothing, radius Ts = smooth_radius in 0..LP_STAB_MAX_SMOOTH, binomial weights: acc = +0.0; for k = -Ts..Ts
 *           in ascending order  acc = acc + (double)C(2 Ts, Ts + k) * s[clamp(t + k, 0, frames - 1)],  the product and the sum
 *           each rounded on its own (no FMA); then sd = acc / 4^Ts (a power of two: exact).
 * stage 5   u = sd + grow.  feather == 0: out = (u > 0) ? 1.0f : 0.0f;  feather > 0: out = (float)min(max(0.5 + u / (2.0 *
 *           feather), 0), 1), the quotient and the sum each rounded on its own.  |grow| <= LP_STAB_MAX_GROW, feather in
 *           0..LP_STAB_MAX_FEATHER, both in pixels.
 * What follows from the rule, at grow = 0: an all-zero video stays exactly 0 and an all-one video exactly 1.0; Tm = Ts = 0 and
 * feather = 0 give the binarised input; a video whose frames are all equal gives that binarised frame for every Tm and Ts at
 * feather = 0; a dropout or a stray blob that lasts at most Tm frames disappears (the smoothing alone does not repair one).  The
 * same bits on every run.
 * lp_mask_signed_d2 is one launch.  lp_mask_stabilize is one launch for stages 2 to 5 (csrc/stabilize_kernel.hip): every lane
 * owns one pixel and marches over t with both windows in registers, so q is read once and out written once.  Where the plane has
 * too few pixels to fill the device the time axis is cut into segments of at least LP_STAB_SEG_FRAMES frames; a segment warms
 * its windows up over the frames in front of it, which cannot change a bit.  No workspace, no floating-point atomics.
 * LP_E_INVALID: null pointer, frames <= 0, a side outside 1..LP_VMASK_MAX_SIDE, a radius outside its range, grow or feather
 * outside its range or NaN, out == q (q == d2 for lp_mask_signed_d2); LP_E_UNSUPPORTED: lp_mask_stabilize with frames > 2^30.
 * All checked before any HIP call.                                                                                             */
#define LP_STAB_Q_FAR       (1 << 30)
#define LP_STAB_MAX_MEDIAN  3
#define LP_STAB_MAX_SMOOTH  8
#define LP_STAB_MAX_GROW    256
#define LP_STAB_MAX_FEATHER 64
#define LP_STAB_SEG_FRAMES  16
#define LP_STAB_SD_CAP      64.0
/*   d2  [frames, 2, height, width] int32 as lp_vmask_edt writes it;  q  out [frames, height, width] int32                      */
LP_API int lp_mask_signed_d2(const int32_t* d2, int32_t frames, int32_t height, int32_t width, int32_t* q, void* stream);

typedef struct lp_stabilize_desc {
    int32_t frames, height, width;
    int32_t median_radius, smooth_radius, reserved0;
    double  grow, feather;
    const int32_t* q;
    float*         out;
} lp_stabilize_desc;
LP_API int lp_mask_stabilize(const lp_stabilize_desc* desc, void* stream);

/* ---- Grain match (beyond the reference) -----------------------------------------------------------------------------------------
 * What the VAE decoder returns under the mask is clean; the photograph or video frame around it carries sensor noise, film grain
 * or compression noise, and on video the clean area reads as a patch that sits still while the grain around it moves.  These four
 * entries measure the grain (lp_grain_stats), turn the two measurements into one amplitude per image, channel and tone band and
 * one grain size per image (lp_grain_fit), and add a synthesized grain under the mask (lp_grain_apply; its noise alone:
 * lp_grain_field).  Last in the chain: ... -> stitch -> multiband blend -> grain match.  Everything stays on the device; nothing is
 * read back.  Exact integers first, then fp64 and fp32 with every operation rounded on its own: the same bits on every run, for
 * every tile, block and chunk.  Sides 1..LP_DETAIL_MAX_SIDE, channels 1..LP_DETAIL_MAX_CHANNELS, batch 1..65535.
 *
 * Kernels  per grain size s = 0, 1, 2 the kernel k_s is the delta, [1 2 1] x [1 2 1] and [1 4 6 4 1] x [1 4 6 4 1], unnormalised.
 *          B3 = k_1.  N3 = [[1,-2,1],[-2,4,-2],[1,-2,1]] (Immerkaer's noise operator, blind to planes); N5 = N3 with its taps two
 *          pixels apart.  With S1_s = sum (N3 * k_s)^2 and S2_s = sum (N5 * k_s)^2:
 *                        s = 0    s = 1    s = 2
 *            sum k^2         1       36     4900
 *            S1             36       36      784
 *            S2             36      784    39204
 *
 * stage 1  lp_grain_stats, integers.  q = the 8-bit codes of image i, channel c, as lp_mask_refine takes them: t = (v > 0) ?
 *          min(v, 1) : 0 (a NaN gives 0), q = (int)(t * 255.0f + 0.5f), product and sum rounded on their own.  Pixel (y, x) takes
 *          part when its 5 x 5 window lies inside the image, max - min of q over that window is <= flat (0..255; 255 keeps
 *          everything: the texture reject), and its region test holds:
 *            LP_GRAIN_REGION_ALL      no mask
 *            LP_GRAIN_REGION_OUTSIDE  every mask element with |y' - y| <= margin and |x' - x| <= margin inside the image is
 *                                     <= 0.5 (lp_color_stats' rule; margin 0..LP_GRAIN_MAX_MARGIN)
 *            LP_GRAIN_REGION_INSIDE   every mask element of the 5 x 5 window is > 0.5
 *          (a NaN in the mask fails either test).  Per pixel mu16 = sum B3 q over the 3 x 3 window (0..4080), band = (mu16 *
 *          LP_GRAIN_BANDS) / 4081 (integer division), e1 = sum N3 q, e2 = sum N5 q.  stats is int64 [batch, channels,
 *          LP_GRAIN_BANDS, 3] = {n, sum e1^2, sum e2^2}.  A side under 5 gives all zeros.  One block per 16 x 64 tile and group
 *          of four channels (codes packed four to a word in LDS); a block adds into 32-bit LDS counters and then into stats with
 *          64-bit integer atomics, after a memset of stats on the same stream: integer sums, the same bits in any order.
 *
 * stage 2  lp_grain_fit, fp64, every operation rounded on its own; one launch, a block per clip.  gen [batch, channels, K, 3]
 *          (the image, LP_GRAIN_REGION_INSIDE) and ref [ref_batch, channels, K, 3] are stage 1 tables.  L = clip_frames (0: L =
 *          batch; L must divide batch); image i belongs to clip i / L.
 *            pool    P = 0.0 + (double)row, the rows of the clip's frames in ascending order, per entry.  ref is pooled over the
 *                    same frames when ref_batch == batch and over all its rows otherwise (a separate grain plate).
 *            energy  per (c, k): valid when P.n >= LP_GRAIN_MIN_COUNT; E_j = P.e_j / P.n.  An invalid band takes E_1, E_2 of the
 *                    nearest valid band of its channel, the lower index on a tie.  A channel without a valid ref band has need
 *                    0; a channel without a valid gen band has Egen = 0.
 *            need    need_j = max(0, Eref_j - Egen_j).
 *            size    size in 0..2 is taken as given.  size == -1: A = sum need_1, Bq = sum need_2 over (c, k) ascending from 0.0;
 *                    A <= 0: size 0 and every amplitude 0;  3 Bq < 14 A: size 0;  else Bq < 33 A: size 1;  else size 2 (the
 *                    geometric means of S2 / S1 of neighbouring sizes).
 *            amp     a = strength * sqrt((need_1 + need_2) / (double)(V * (S1_s + S2_s))), V = LP_GRAIN_WHITE_VAR;
 *                    a = min(a, LP_GRAIN_MAX_STD / sqrt((double)(V * sum k_s^2)));  amp = (float)(a / 255.0).
 *          amp is fp32 [batch, channels, K], size int32 [batch]; every frame of a clip gets its clip's values.
 *
 * field    w(frame, y, x, c), -2 <= y < height + 2, -2 <= x < width + 2: the Philox4x32-10 block (Random123) with counter
 *          ((y + 2) * (width + 4) + (x + 2) [64 bit], frame * 16 + c / 4 [64 bit]) and key seed; of its word c % 4, the sum of
 *          the four bytes minus 510 (variance LP_GRAIN_WHITE_VAR = 4 * (256^2 - 1) / 12).  monochrome: c = 0 for every channel.
 *          frame = frame0 + i.  g = sum k_s(dy, dx) w(y + dy, x + dx), an exact integer that depends on (seed, frame, y, x, c,
 *          width, s) only.  lp_grain_field writes g as int32 [batch, height, width, channels].
 *
 * stage 3  lp_grain_apply, fp32, every operation rounded on its own.  mu16 as in stage 1 but with coordinates clamped to the
 *          image, on `image`; K = LP_GRAIN_BANDS:
 *            u = min(max((float)(mu16 * K) / 4080.0f - 0.5f, 0), K - 1);  k0 = min((int)u, K - 2);  f = u - (float)k0
 *            a = amp[k0] + f * (amp[k0 + 1] - amp[k0]);  m = (mask > 0) ? min(mask, 1) : 0 (a NaN gives 0);  t = m * a
 *            out = image + t * (float)g, and where t == 0 out is image's bits (no clamp of the result)
 *          s = size[i], read on the device.  One launch: a block per 16 x 64 tile and group of four channels computes each white
 *          value of its lattice once (one Philox block serves four channels), filters along x and then along y through LDS.
 *
 * LP_E_INVALID: null pointer, batch <= 0, a side or the channel count outside the limits, mask_batch not 1 or batch, margin,
 * flat, region, size, strength (NaN included), clip_frames < 0 or not a divisor of batch, ref_batch <= 0, frame0 outside
 * 0..LP_GRAIN_MAX_FRAME0, out == image; LP_E_UNSUPPORTED: batch (or ref_batch) > 65535.  All checked before any HIP call.          */
#define LP_GRAIN_BANDS      8
#define LP_GRAIN_MIN_COUNT  64
#define LP_GRAIN_WHITE_VAR  21845
#define LP_GRAIN_MAX_STD    64
#define LP_GRAIN_MAX_MARGIN 25
#define LP_GRAIN_TILE_H     16
#define LP_GRAIN_TILE_W     64
#define LP_GRAIN_REGION_ALL     0
#define LP_GRAIN_REGION_OUTSIDE 1
#define LP_GRAIN_REGION_INSIDE  2
#define LP_GRAIN_SIZE_AUTO  -1
#define LP_GRAIN_MAX_FRAME0 (1 << 30)

typedef struct lp_grain_stats_desc {
    int32_t batch, height, width, channels;
    int32_t mask_batch, margin, flat, region;
    const float* image;     /* [batch, height, width, channels] fp32                                             */
    const float* mask;      /* [mask_batch, height, width] fp32; may be null with LP_GRAIN_REGION_ALL               */
    int64_t*     stats;     /* out, [batch, channels, LP_GRAIN_BANDS, 3]                                          */
} lp_grain_stats_desc;
LP_API int lp_grain_stats(const lp_grain_stats_desc* desc, void* stream);

typedef struct lp_grain_fit_desc {
    int32_t batch, ref_batch, channels, clip_frames;
    int32_t size, reserved0;      /* LP_GRAIN_SIZE_AUTO or 0..2                                                  */
    double  strength;             /* 0..2                                                                        */
    const int64_t* gen;
    const int64_t* ref;
    float*   amp;                 /* out, [batch, channels, LP_GRAIN_BANDS]                                       */
    int32_t* size_out;            /* out, [batch]                                                                */
} lp_grain_fit_desc;
LP_API int lp_grain_fit(const lp_grain_fit_desc* desc, void* stream);

typedef struct lp_grain_field_desc {
    int32_t  batch, height, width, channels;
    int32_t  size, monochrome;    /* size 0..2                                                                   */
    int64_t  frame0;
    uint64_t seed;
    int32_t* out;                 /* [batch, height, width, channels]                                            */
} lp_grain_field_desc;
LP_API int lp_grain_field(const lp_grain_field_desc* desc, void* stream);

typedef struct lp_grain_apply_desc {
    int32_t  batch, height, width, channels;
    int32_t  mask_batch, monochrome;
    int64_t  frame0;
    uint64_t seed;
    const float*   image;         /* [batch, height, width, channels] fp32                                       */
    const float*   mask;          /* [mask_batch, height, width] fp32                                            */
    const float*   amp;           /* [batch, channels, LP_GRAIN_BANDS] (lp_grain_fit)                            */
    const int32_t* size;          /* [batch], each 0..2 (lp_grain_fit)                                           */
    float*         out;           /* [batch, height, width, channels]                                            */
} lp_grain_apply_desc;
LP_API int lp_grain_apply(const lp_grain_apply_desc* desc, void* stream);

/* ---- Video mask propagate (beyond the reference) ----------------------------------------------------------------------------------
 * One mask painted on one frame of a clip follows the picture's motion through the other frames.  The video mask editor morphs
 * between painted keyframes and follows a subject's centroid, not its outline; the stabilize is not motion-compensated.  These
 * entries are the first link of the chain:  one painted mask + the video -> propagate -> stabilize -> refine -> encode / Detailer
 * crops.  A block matching, weighted by the mask, measures the motion from a frame s to the next frame t (one frame further from
 * the key); a map of key-frame positions is carried along that motion and the key mask is sampled through it.  Everything stays on
 * the device; nothing is read back.  All of it is integer arithmetic: the same bits on every run, for every tile and every chunk
 * of frames.  Several keyframes: the lp_prop_*_batch section below.  Not handled: occlusion.
 *   sides 1..LP_VMASK_MAX_SIDE; levels L in 1..LP_PROP_MAX_LEVELS; search R in 1..LP_PROP_MAX_SEARCH; smooth 0..LP_PROP_MAX_SMOOTH
 *   B = LP_PROP_BLOCK = 8; a block's window is the block grown by LP_PROP_HALO = 4 on every side and cut at the image border (at
 *   most 16 x 16); vectors and positions are in units of 1 / LP_PROP_SUBPEL = 1/16 pixel, (y, x) pairs of int32.  `>>` is the
 *   arithmetic shift (a floor); clamp(i) holds a coordinate inside its plane.
 *
 * 1 luma      The 8-bit codes of image values are taken as lp_mask_refine takes them: t = (v > 0) ? min(v, 1) : 0 (a NaN gives 0),
 *             code = (int)(t * 255.0f + 0.5f), product and sum rounded on their own.  channels >= 3: Y = (77 R + 150 G + 29 B +
 *             128) >> 8 on the first three channels; channels 1 or 2: Y = the code of channel 0.  uint8 [frames, height, width].
 * 2 pyramids  Level l + 1 of a plane of h x w is ceil(h / 2) x ceil(w / 2); pixel (y, x) is (a + b + c + d + 2) >> 2 of the luma
 *             at (clamp(2y + i), clamp(2x + j)), i, j in {0, 1}, of the level below.  The mask pyramid of a frame is the OR of
 *             the mask bits over the same footprints.  Level l of a height x width plane is ceil(height / 2^l) x ceil(width / 2^l).
 *             A frame's pyramid is one byte string: level l, row-major, starts LP_PROP_ALIGN-aligned behind level l - 1;
 *             lp_prop_pyramid_ws_bytes(1, ...) is a frame's stride.
 * 3 one step  s -> t with the mask bits m of s known, levels l = L - 1 down to 0, on the grid of ceil(h_l / 8) x ceil(w_l / 8) blocks:
 *   predictor p (integer pixels): 0 at level L - 1, else per component p = 2 * ((v + 8) >> 4) of the final vector v of the parent
 *             block (by >> 1, bx >> 1), clamped to the parent's grid.
 *   valid     the block's window holds at least LP_PROP_MIN_PIXELS = 16 mask pixels of this level.
 *   match     (lp_prop_match; valid blocks) for oy, ox in -R..R in raster order, idx = (oy + R) (2R + 1) + ox + R:
 *             S(oy, ox) = sum over the window's mask pixels (y, x) of |Ys(y, x) - Yt(clamp(y + py + oy), clamp(x + px + ox))|,
 *             cost = S + smooth * (|oy| + |ox|); the winner has the least key = cost << 12 | (|oy| + |ox|) << 8 | idx, and
 *             v = 16 (p + o).  S <= 256 * 255 and cost < 2^17, so the key stays inside 32 bits.
 *             Level 0 only, per axis, when the winner is not at -R or R on that axis and S0 = S(winner) != 0: with cm, cp the S
 *             one step below and above on that axis and d = cm + cp - 2 S0:  d <= 0 adds nothing, else v += sign(cm - cp) *
 *             min(|8 (cm - cp)| / d, 8), the division truncating.  (S0 == 0 adds nothing: a noise-free whole-pixel shift and a
 *             still video are tracked exactly.)  An invalid block holds v = 16 p.
 *   fill      (lp_prop_fill) LP_PROP_FILL_ITERS = 3 Jacobi passes: an invalid block with n >= 1 valid blocks among its 3 x 3
 *             neighbours inside the grid takes per component floor((2 sum + n) / (2 n)) of their vectors and becomes valid for
 *             the next pass.  Blocks still invalid keep 16 p: an empty mask gives the zero field without any read-back.
 *   median    then per component the median of the 3 x 3 neighbourhood, the border replicated: the level's final field.
 *   per pixel (lp_prop_advance, level 0) per axis u = 2x - 7, b0 = u >> 4, f = u - 16 b0, blocks b0 and b0 + 1 clamped to the grid;
 *             V = ((16 - fy) * ((16 - fx) v00 + fx v01) + fy * ((16 - fx) v10 + fx v11) + 128) >> 8.
 *   advance   P_key(y, x) = (16 y, 16 x).  P_t(y, x) = (bil(P_s, 16 y - Vy, 16 x - Vx) + 128) >> 8 per component, where bil(A, qy,
 *             qx) clamps q to 0..16 (n - 1) per axis, i = q >> 4, f = q & 15, i1 = min(i + 1, n - 1) and returns (16 - fy) * ((16 -
 *             fx) A[iy, ix] + fx A[iy, ix1]) + fy * ((16 - fx) A[iy1, ix] + fx A[iy1, ix1]).  The mask code of t is c = bil(b, P_t)
 *             in 0..256 with b the key mask binarised at >= 0.5 (a NaN gives 0); out = c / 256 as fp32; the bits that weight the
 *             next step are c >= 128.  Positions are below 2^18 and their weighted sums below 2^26: inside an int32.
 * The frames behind the key and the frames in front of it are two independent chains that start from the key.  The key frame's own
 * output is its binarised mask (lp_prop_key_mask).  What follows from the rule: one frame returns the binarised mask; an empty
 * mask gives exactly 0 and a full mask exactly 1.0 on every frame; a video of equal frames returns the binarised key mask on every
 * frame.
 * Launches (csrc/propagate_kernel.hip): lp_prop_luma 1 + (levels - 1) for all its frames; lp_prop_key_mask, lp_prop_match,
 * lp_prop_fill and lp_prop_advance one each, so a step is 2 L + 1 launches.  lp_prop_match: one wave per block; the source window,
 * its per-byte mask and the (16 + 2R)^2 target patch in LDS, the candidates over the lanes, v_sad_u8 on four pixels at a time.
 * LP_E_INVALID: null pointer, a side, levels, level, search, smooth, channels or grid outside its range, frames <= 0, parent null
 * below the top level or not null at it, pos_dst == pos_src; LP_E_UNSUPPORTED: frames > 65535.  All checked before any HIP call. */
#define LP_PROP_BLOCK       8
#define LP_PROP_HALO        4
#define LP_PROP_MIN_PIXELS  16
#define LP_PROP_FILL_ITERS  3
#define LP_PROP_SUBPEL      16
#define LP_PROP_MAX_LEVELS  6
#define LP_PROP_MAX_SEARCH  7
#define LP_PROP_MAX_SMOOTH  64
#define LP_PROP_ALIGN       16
#define LP_PROP_MAX_GRID    2048   /* ceil(LP_VMASK_MAX_SIDE / LP_PROP_BLOCK) */

/* Bytes of `frames` pyramids of `levels` levels of a height x width uint8 plane (stage 2's layout); frames = 1 gives one frame's
 * stride.  Host arithmetic, no HIP call.  LP_E_INVALID for frames <= 0, a side or levels outside its range.                      */
LP_API int64_t lp_prop_pyramid_ws_bytes(int32_t frames, int32_t height, int32_t width, int32_t levels);

typedef struct lp_prop_luma_desc {
    int32_t frames, height, width, channels;      /* channels 1..LP_DETAIL_MAX_CHANNELS                                     */
    int32_t levels, reserved0;
    const float* image;                           /* [frames, height, width, channels] fp32                                 */
    uint8_t*     pyramid;                         /* out, lp_prop_pyramid_ws_bytes(frames, height, width, levels) bytes      */
} lp_prop_luma_desc;
LP_API int lp_prop_luma(const lp_prop_luma_desc* desc, void* stream);

/* mask [height, width] fp32 -> its bits' pyramid (one frame, values 0 / 1) and, unless null, out [height, width] = the bits as fp32 */
LP_API int lp_prop_key_mask(const float* mask, int32_t height, int32_t width, int32_t levels, uint8_t* mask_pyramid, float* out,
                            void* stream);

typedef struct lp_prop_match_desc {
    int32_t height, width, levels, level;         /* height, width: level 0's                                               */
    int32_t search, smooth;
    const uint8_t* src;                           /* the luma pyramid of frame s (its level 0's address)                    */
    const uint8_t* tgt;                           /* the luma pyramid of frame t                                            */
    const uint8_t* mask;                          /* the mask pyramid of frame s                                            */
    const int32_t* parent;                        /* level + 1's final field [gh', gw', 2]; null exactly at level levels - 1 */
    int32_t*       vec;                           /* out, [gh, gw, 2]                                                       */
    int32_t*       valid;                         /* out, [gh, gw], 0 / 1                                                   */
} lp_prop_match_desc;
LP_API int lp_prop_match(const lp_prop_match_desc* desc, void* stream);

/* fill and median of one level: vec [grid_h, grid_w, 2], valid [grid_h, grid_w] as lp_prop_match wrote them -> out, the final field;
 * out != vec.  grid sides 1..LP_PROP_MAX_GRID.                                                                                     */
LP_API int lp_prop_fill(const int32_t* vec, const int32_t* valid, int32_t grid_h, int32_t grid_w, int32_t* out, void* stream);

typedef struct lp_prop_advance_desc {
    int32_t height, width, levels, reserved0;
    const int32_t* vec;                           /* level 0's final field                                                  */
    const int32_t* pos_src;                       /* P_s [height, width, 2]; null: P_key                                    */
    const uint8_t* key;                           /* the key mask's bits [height, width] (level 0 of its pyramid)           */
    int32_t*       pos_dst;                       /* out, P_t; != pos_src                                                   */
    float*         out;                           /* out, [height, width] fp32                                              */
    uint8_t*       mask_pyramid;                  /* out, the pyramid of frame t's bits                                     */
} lp_prop_advance_desc;
LP_API int lp_prop_advance(const lp_prop_advance_desc* desc, void* stream);

/* ---- Video mask propagate from several keyframes (beyond the reference) -----------------------------------------------------------
 * One chain loses accuracy with its distance from the key, and a user who repaints a later frame wants both paintings honoured.
 * With several painted keys every key is carried along the picture's motion in both directions; between two keys the two carried
 * masks are merged through their signed distance fields with weights that move from one key to the other, so the result equals
 * the painted mask on every key frame and drift is pulled back to zero there.
 *   inputs    key frames k_0 < k_1 < ... < k_{K-1} in 0..F-1, a painted mask per key, the lp_prop_* parameters unchanged.
 *   chains    each chain is exactly stages 1 to 3 of the section above started from one key, in this order: backward from k_0 to
 *             frame 0 if k_0 > 0; per gap i = 0..K-2 forward from k_i to k_{i+1} - 1, then backward from k_{i+1} to k_i + 1;
 *             forward from k_{K-1} to F - 1 if it is not the last frame.  A chain of length 0 does not exist.  Chain c with key k
 *             and direction d = +-1 goes at step s >= 1 from frame k + d (s - 1) to frame k + d s.
 *   output    a key frame gets its binarised painted mask, as lp_prop_key_mask writes it; a frame outside [k_0, k_{K-1}] gets its
 *             one chain's output c / 256; a frame t strictly inside a gap (a, b) gets the merge of A, the forward chain's output
 *             at t, and B, the backward chain's, with n = b - a and j = t - a.
 *   merge     (lp_prop_merge) qA, qB: the signed squared distances of A and B binarised at >= 0.5, exactly as lp_mask_signed_d2
 *             defines them, +-LP_STAB_Q_FAR on an empty or a full frame.  sX = sign(qX) * sqrt((double)|qX|), the correctly rounded
 *             fp64 root, capped at +-LP_STAB_SD_CAP exactly as stage 3 of lp_mask_stabilize.  acc = (double)(n - j) * sA +
 *             (double)j * sB, the two products and the sum each rounded on its own (no FMA); sd = acc / (double)n;
 *             out = (float)min(max(0.5 + sd, 0.0), 1.0).
 * What follows from the rule: where A and B have the same bits the output is exactly those bits, since |s| >= 1 puts 0.5 + sd
 * beyond the ramp; K = 1 is the single-key propagate, bit for bit; a still video with the same mask on every key returns that
 * binarised mask on every frame; empty masks everywhere stay exactly 0 and full masks everywhere exactly 1.0.  An empty key next to
 * a non-empty one says "nothing here": its distance is the cap, 64, which outweighs a small object's depth, so the other key's mask
 * appears only in the last frames before that key.  This is deliberate.  The same bits on every run.
 * The up to 2 K chains do not depend on one another: lp_prop_match_batch, lp_prop_fill_batch and lp_prop_advance_batch run up to
 * LP_PROP_MAX_JOBS independent chain steps in one launch, the job on blockIdx.z, every job with the meaning and the bits of the
 * single entry (the single entries are one-job batches of the same kernels).  The job table is read from host memory and travels
 * by value in the kernel's arguments (32 x 48 bytes); no device table is uploaded.  A call has as many dependent steps as its longest
 * chain, each 2 L + 1 launches per 32 active chains.  Two jobs that write the same buffer are the caller's error; nothing checks it.
 * LP_E_INVALID: jobs outside 1..LP_PROP_MAX_JOBS; a null pointer, except parent at the top level and pos_src; parent given at the
 * top level or missing below it, in any job; out == vec, pos_dst == pos_src or mask_pyramid == key within a job; every range the
 * single entries check.  lp_prop_merge: a null pointer, a side outside 1..LP_VMASK_MAX_SIDE, span < 2, first < 1, frames < 1,
 * first + frames - 1 > span - 1, out aliasing qa or qb; LP_E_UNSUPPORTED: span > 65535.  All checked before any HIP call.            */
#define LP_PROP_MAX_JOBS    32
#define LP_PROP_MATCH_WARPED_KEY 1                /* lp_prop_match_batch_desc.reserved0: the several-keys anchored section  */
/* reserved0 of the gated warped-key form, occlusion 1..255 in bits 8..15: the several-keys anchored occlusion-aware section */
#define LP_PROP_MATCH_GATED(occlusion) (LP_PROP_MATCH_WARPED_KEY | ((occlusion) << 8))

typedef struct lp_prop_match_job {
    const uint8_t* src;                           /* as in lp_prop_match_desc                                               */
    const uint8_t* tgt;
    const uint8_t* mask;
    const int32_t* parent;
    int32_t*       vec;
    int32_t*       valid;
} lp_prop_match_job;

typedef struct lp_prop_match_batch_desc {
    int32_t height, width, levels, level;
    int32_t search, smooth;
    int32_t jobs, reserved0;                      /* jobs 1..LP_PROP_MAX_JOBS; reserved0 is the source form: 0 the source
                                                     frame's luma, LP_PROP_MATCH_WARPED_KEY the key frame's luma warped
                                                     through the job's positions (the several-keys anchored section),
                                                     LP_PROP_MATCH_GATED(occlusion) that with the occlusion gate           */
    const lp_prop_match_job* job;                 /* host memory, `jobs` entries                                            */
} lp_prop_match_batch_desc;
LP_API int lp_prop_match_batch(const lp_prop_match_batch_desc* desc, void* stream);

typedef struct lp_prop_fill_job {
    const int32_t* vec;                           /* as lp_prop_fill's arguments; out != vec                                */
    const int32_t* valid;
    int32_t*       out;
} lp_prop_fill_job;
/* job: host memory, `jobs` entries, every job's grid grid_h x grid_w                                                      */
LP_API int lp_prop_fill_batch(const lp_prop_fill_job* job, int32_t jobs, int32_t grid_h, int32_t grid_w, void* stream);

typedef struct lp_prop_advance_job {
    const int32_t* vec;                           /* as in lp_prop_advance_desc; a null pos_src means P_key                 */
    const int32_t* pos_src;
    const uint8_t* key;
    int32_t*       pos_dst;
    float*         out;
    uint8_t*       mask_pyramid;
} lp_prop_advance_job;

typedef struct lp_prop_advance_batch_desc {
    int32_t height, width, levels, jobs;
    const lp_prop_advance_job* job;               /* host memory, `jobs` entries                                            */
} lp_prop_advance_batch_desc;
LP_API int lp_prop_advance_batch(const lp_prop_advance_batch_desc* desc, void* stream);

/* The in-between frames of one gap: frame f of the stacks is frame j = first + f of the gap, 1 <= j <= span - 1.  One launch. */
typedef struct lp_prop_merge_desc {
    int32_t frames, height, width, span;          /* span = n, the distance between the two keys                            */
    int32_t first, reserved0;
    const int32_t* qa;                            /* [frames, height, width] signed squared distances of the forward chain  */
    const int32_t* qb;                            /* the same of the backward chain                                         */
    float*         out;                           /* [frames, height, width] fp32                                           */
} lp_prop_merge_desc;
LP_API int lp_prop_merge(const lp_prop_merge_desc* desc, void* stream);

/* ---- Video mask propagate, occlusion-aware (beyond the reference) ------------------------------------------------------------------
 * When the masked subject passes behind something, the carried mask of the single-key section lies on what is in front, and the
 * sampler repaints it.  The position map P_t names, for every pixel of frame t, where it was in the key frame; sampling the key
 * frame's luma through it shows what the subject should look like there.  Where the picture of t looks different, something is in
 * front: that part of the mask is taken out and returned separately as `hidden`.  A step of this form is the single-key step with
 * two launches behind it (the existing entries keep their meaning and their bits):
 *   lp_prop_match / lp_prop_fill per level -> lp_prop_advance (its out and mask_pyramid go to scratch) -> lp_prop_visible ->
 *   lp_prop_occlude.
 * All of it is integer arithmetic.  For frame t after lp_prop_advance: c(y, x) in 0..256 the advance's mask code, m = c >= 128
 * (level 0 of the pyramid the advance wrote), P_t the positions, Yt and Yk level 0 of the luma pyramids of t and of the key frame;
 * bil, the block grid, the window, LP_PROP_BLOCK, LP_PROP_HALO and LP_PROP_MIN_PIXELS as in the single-key section.
 * 1 warped key luma  K(y, x) = (bil(Yk, P_t(y, x)) + 128) >> 8, in 0..255;  d = Yt(y, x) - K(y, x).
 * 2 per block  (lp_prop_visible) M: the pixels of the block's window with m = 1, n = |M|.  n < LP_PROP_MIN_PIXELS: the flag is 0
 *              (no evidence: the block counts as visible).  Else D = sum over M of d; mu = floor((2 D + n) / (2 n)), the
 *              mathematical floor, clamped to +-LP_PROP_VIS_MAX_BIAS = 32 (an exposure change is forgiven, a dark object in front
 *              of a bright one is not); R = sum over M of |d - mu|; the flag is 1 (occluded) iff R > occlusion * n, with occlusion
 *              in 1..255 the mean residual in grey levels.  |D| and R stay below 2^17.  flags: int32 [gh, gw].
 * 3 per pixel  (lp_prop_occlude) v = 1 - flag; w in 0..256 is v interpolated over the blocks exactly as lp_prop_advance
 *              interpolates the field: per axis u = 2x - 7, b0 = u >> 4, f = u - 16 b0, blocks b0 and b0 + 1 clamped to the grid,
 *              w = (16 - fy) * ((16 - fx) v00 + fx v01) + fy * ((16 - fx) v10 + fx v11).  c' = (c * w + 128) >> 8;
 *              mask = c' / 256 and hidden = (c - c') / 256, both fp32 and exact; the bits that weight the next step's match are
 *              c' >= 128, and their pyramid is written as lp_prop_advance writes its own.  c is read back from the advance's out:
 *              c = (int)(out * 256), exact, held inside 0..256.
 * 4 no memory between frames: the test is against the key in every frame, so a part that was hidden is visible again as soon as
 *   its residual drops.  Blocks whose bits are gone are invalid in the next match and are filled from their valid neighbours (the
 *   existing rule): the hidden part's positions follow the visible rest.  A subject that is hidden entirely leaves the zero field;
 *   if it reappears elsewhere it is lost.
 * 5 the key frame's own output is its binarised mask (lp_prop_key_mask), its hidden is 0.
 * What follows from the rule, bit for bit: a video of equal frames returns the binarised key mask and an all-zero hidden for every
 * occlusion >= 1 (d = 0 everywhere, w = 256); so does a noise-free whole-pixel shift away from the border; an empty mask gives 0
 * and 0; mask + hidden = c / 256 on every frame where the chain's bits so far equal the plain chain's.  occlusion = 0 is the
 * caller's "off": it makes neither launch and returns the plain chain and zeros.
 * Launches (csrc/propagate_kernel.hip): lp_prop_visible, a block of 256 lanes per 32 x 32 pixels: d of the tile and its halo of 4
 * goes to LDS once as int16 (a pixel outside the image or the mask holds a marker), four pixels per lane with P_t read as two
 * 16-byte vectors when width % 4 == 0; then 16 lanes per window, a row each, D and n and then R summed across them in registers.
 * lp_prop_occlude: a block per 32 x 32 tile, one lane per four pixels, ending in the pyramid's tile code.  One job each
 * (one-job batches of the next section's kernels).
 * LP_E_INVALID: a null pointer, a side or levels outside its range, occlusion outside 1..255, flags aliasing an input of
 * lp_prop_visible; out, hidden or mask_pyramid aliasing code or flags or one another in lp_prop_occlude (the advance's pyramid is
 * no input there: c carries its bits, so mask_pyramid may not be the buffer lp_prop_visible still reads, which the caller orders).
 * All checked before any HIP call.                                                                                                  */
#define LP_PROP_VIS_MAX_BIAS 32

typedef struct lp_prop_visible_desc {
    int32_t height, width, occlusion, reserved0;  /* occlusion 1..255                                                       */
    const int32_t* pos;                           /* P_t [height, width, 2], as lp_prop_advance wrote it                    */
    const uint8_t* tgt;                           /* Yt: level 0 of frame t's luma pyramid [height, width]                  */
    const uint8_t* key;                           /* Yk: level 0 of the key frame's luma pyramid                            */
    const uint8_t* mask;                          /* m: level 0 of the pyramid lp_prop_advance wrote                        */
    int32_t*       flags;                         /* out, [gh, gw], 0 visible / 1 occluded                                  */
} lp_prop_visible_desc;
LP_API int lp_prop_visible(const lp_prop_visible_desc* desc, void* stream);

typedef struct lp_prop_occlude_desc {
    int32_t height, width, levels, reserved0;
    const float*   code;                          /* c / 256 [height, width]: lp_prop_advance's out                         */
    const int32_t* flags;                         /* [gh, gw] as lp_prop_visible wrote them                                 */
    float*         out;                           /* out, mask = c' / 256 [height, width]                                   */
    float*         hidden;                        /* out, (c - c') / 256 [height, width]                                    */
    uint8_t*       mask_pyramid;                  /* out, the pyramid of the bits c' >= 128                                 */
} lp_prop_occlude_desc;
LP_API int lp_prop_occlude(const lp_prop_occlude_desc* desc, void* stream);

/* ---- Video mask propagate from several keyframes, occlusion-aware (beyond the reference) ---------------------------------------------
 * The several-keys section has no occlusion handling and the occlusion-aware section has one key: a subject that is hidden entirely
 * is lost there.  The remedy is a second key painted behind the occluder.  This section joins the two, and adds the rule the join
 * needs: between two keys, the chain that went through a full occlusion is stale, and a merge weighted by time alone would drag the
 * good chain towards it.  A chain that is lost gives way to the other.
 * 1 chains   the plan of the several-keys section, unchanged.  Every chain is the occlusion-aware chain of the section above started
 *            from its own key: match / fill per level -> advance -> visible (Yk is that chain's key frame's luma) -> occlude.  For
 *            chain X at frame t this gives the advance's code c_X, the visible code c'_X and the flags f_X [gh, gw] on frame t's block
 *            grid.  The subject code is c_X; hidden_X = (c_X - c'_X) / 256.
 * 2 lost     N_X(u) is the number of pixels with c'_X >= 128 at frame u; at the key itself, the number of key bits.  Chain X is lost
 *            at t if N_X(key) >= LP_PROP_MIN_PIXELS and N_X(u) < LP_PROP_MIN_PIXELS for some frame u from its first step up to t
 *            inclusive: below 16 visible bits no level-0 block of the next match can be valid.  A chain from a key with fewer than
 *            16 bits is never lost: an empty key keeps its "nothing here" meaning.  Lost is sticky along the chain; the chain still
 *            runs on.
 * 3 output   a key frame gets its binarised painted mask and hidden = 0.  A frame outside [k_0, k_{K-1}] gets its one chain's
 *            (c' / 256, (c - c') / 256), lost or not.  A frame t strictly inside a gap (a, b), n = b - a, j = t - a, with A the forward
 *            and B the backward chain (lp_prop_merge_visible):
 *              exactly one of A, B lost at t: the other chain's mask and hidden, bit for bit.
 *              otherwise (none or both lost): S = the lp_prop_merge value of qA and qB, the signed squared distances of c_A >= 128
 *              and of c_B >= 128 (the subject codes, not the visible parts), the arithmetic exactly lp_prop_merge's;
 *              c_S = (int)(S * 256.0f + 0.5f), product and sum rounded on their own, in 0..256; f = f_A if 2 j <= n, else f_B (the
 *              nearer key's verdict); w = f interpolated exactly as lp_prop_occlude does; c'_S = (c_S * w + 128) >> 8;
 *              mask = c'_S / 256 and hidden = (c_S - c'_S) / 256.
 * What follows from the rule, bit for bit: K = 1 is the occlusion-aware single-key form; occlusion = 0 is the caller's "off" (the
 * several-keys form and a zero hidden, none of this section's launches); a still video with the same mask on every key returns
 * the binarised mask and a zero hidden on every frame; empty keys everywhere give 0 and 0; mask + hidden is a multiple of 1 / 256
 * everywhere; on every key the output is the painting.
 * lp_prop_visible_batch and lp_prop_occlude_batch run up to LP_PROP_MAX_JOBS independent chain steps in one launch, the job on
 * blockIdx.z, the job table read from host memory and passed by value, every job with the meaning and the bits of the single entry
 * (the single entries are one-job batches of the same kernels; a job takes the 16-byte paths when its own planes allow).  A step of
 * this form is 2 L + 3 launches per 32 active chains.  An occlude job with a count adds the number of its pixels with c' >= 128
 * to *count (int32, zeroed by the caller): one integer atomic add per wave, so any order gives the same bits.  count null: none.
 * lp_prop_merge_visible: one launch per gap, or per chunk of its frames through `first`; a streaming kernel, four pixels per lane
 * in 16-byte accesses when width % 4 == 0 and the planes are 16-byte aligned, one pixel per lane otherwise, the same bits.  The
 * two lost bits of a frame are derived on the device from the chains' counts, which are indexed by the chain's step (index 0 the
 * key's count, count_a[j] frame a + j, count_b[s] frame b - s), span entries each, whatever `first` is: nothing is read back.
 * out may be mask_a and hidden may be code_a (in place on the forward chain's planes; a lane reads its pixels before it writes).
 * LP_E_INVALID: jobs outside 1..LP_PROP_MAX_JOBS; per job every check of the single entries; a count that aliases another pointer
 * of its job.  lp_prop_merge_visible: a null pointer, a side outside 1..LP_VMASK_MAX_SIDE, span < 2, first < 1, frames < 1,
 * first + frames - 1 > span - 1, out == hidden, out or hidden aliasing an input other than the in-place pair; LP_E_UNSUPPORTED:
 * span > 65535.  All checked before any HIP call.                                                                                 */
typedef struct lp_prop_visible_job {
    const int32_t* pos;                           /* as in lp_prop_visible_desc                                             */
    const uint8_t* tgt;
    const uint8_t* key;
    const uint8_t* mask;
    int32_t*       flags;
} lp_prop_visible_job;

typedef struct lp_prop_visible_batch_desc {
    int32_t height, width, occlusion, jobs;       /* occlusion 1..255, jobs 1..LP_PROP_MAX_JOBS                             */
    const lp_prop_visible_job* job;               /* host memory, `jobs` entries                                            */
} lp_prop_visible_batch_desc;
LP_API int lp_prop_visible_batch(const lp_prop_visible_batch_desc* desc, void* stream);

typedef struct lp_prop_occlude_job {
    const float*   code;                          /* as in lp_prop_occlude_desc                                             */
    const int32_t* flags;
    float*         out;
    float*         hidden;
    uint8_t*       mask_pyramid;
    int32_t*       count;                         /* += the number of pixels with c' >= 128; null: not counted              */
} lp_prop_occlude_job;

typedef struct lp_prop_occlude_batch_desc {
    int32_t height, width, levels, jobs;
    const lp_prop_occlude_job* job;               /* host memory, `jobs` entries                                            */
} lp_prop_occlude_batch_desc;
LP_API int lp_prop_occlude_batch(const lp_prop_occlude_batch_desc* desc, void* stream);

/* The in-between frames of one gap: frame f of the stacks is frame j = first + f of the gap, 1 <= j <= span - 1.  One launch. */
typedef struct lp_prop_merge_visible_desc {
    int32_t frames, height, width, span;          /* span = n, the distance between the two keys                            */
    int32_t first, reserved0;
    const int32_t* qa;                            /* [frames, height, width] signed squared distances of c_A >= 128         */
    const int32_t* qb;                            /* the same of c_B >= 128                                                 */
    const float*   code_a;                        /* [frames, height, width] c_A / 256: the forward chain's advance         */
    const float*   mask_a;                        /* c'_A / 256: its occlude's out                                          */
    const float*   code_b;                        /* the same two of the backward chain                                     */
    const float*   mask_b;
    const int32_t* flags_a;                       /* [frames, gh, gw] f_A                                                   */
    const int32_t* flags_b;                       /* f_B                                                                    */
    const int32_t* count_a;                       /* [span] N_A by step: [0] the key's bits, [j] frame a + j                */
    const int32_t* count_b;                       /* [span] N_B by step: [0] the key's bits, [s] frame b - s                */
    float*         out;                           /* [frames, height, width] mask                                           */
    float*         hidden;                        /* [frames, height, width]                                                */
} lp_prop_merge_visible_desc;
LP_API int lp_prop_merge_visible(const lp_prop_merge_visible_desc* desc, void* stream);

/* ---- Video mask propagate, anchored (beyond the reference) ---------------------------------------------------------------------------
 * The single-key chain composes one-frame fields.  Every step's sub-pixel estimate is pulled towards zero by `smooth` and by the
 * parabola fit, and nothing ever looks at the key frame again, so on a long clip with sub-pixel motion the mask falls behind its
 * subject.  The position map P_t names, for every pixel of frame t, where it was in the key frame; the key frame's luma sampled
 * through it is the picture the chain believes frame t to be.  Matched against the real frame t with the block-match rule, the block
 * field is the error the chain has built up, and one more advance along it takes the error out.  The match is against the key every
 * time, so the error no longer accumulates.  A step of this form is the single-key step with three launches behind it (the existing
 * entries keep their meaning and their bits):
 *   lp_prop_match / lp_prop_fill per level -> lp_prop_advance (its out and mask_pyramid go to scratch) -> lp_prop_anchor_match ->
 *   lp_prop_fill -> lp_prop_advance.
 * All of it is integer arithmetic.  For frame t after the first lp_prop_advance: c(y, x) in 0..256 the advance's mask code,
 * m = c >= 128 (level 0 of the pyramid the advance wrote), P_t the positions, Yt and Yk level 0 of the luma pyramids of t and of the
 * key frame; everything else as in the single-key section.
 * 1 warped key luma  K(y, x) = (bil(Yk, P_t(y, x)) + 128) >> 8, in 0..255: exactly lp_prop_visible's K.
 * 2 correction field (lp_prop_anchor_match) e [gh, gw, 2] is step 3's `match` at level 0 of the single-key section with Ys := K,
 *              Yt := Yt, the mask := m, the predictor p = 0, search := anchor in 1..LP_PROP_MAX_SEARCH, the chain's smooth, and the
 *              level-0 sub-pixel refinement: the same window (the block grown by LP_PROP_HALO, cut at the border), validity
 *              (LP_PROP_MIN_PIXELS), key order and clamping of target coordinates.  An invalid block holds 0.
 * 3 fill       the existing lp_prop_fill (fill + median) on e.
 * 4 advance    the existing lp_prop_advance with vec = e, pos_src = P_t and the key bits: its pos_dst, out and mask_pyramid are the
 *              step's results, the positions, the mask and the bits that weight the next step's match.
 * 5 no memory between frames except P_t itself; the key frame's own output is its binarised mask (lp_prop_key_mask).
 * What follows from the rule, bit for bit: a video of equal frames gives e = 0 on every frame and the plain chain's bits, and so
 * does a noise-free whole-pixel shift that the plain chain tracks exactly (K = Yt under the mask, S = 0 at the zero vector, which
 * every other candidate can only tie at a larger distance); an empty mask gives 0 and a full mask 1.0; one frame returns the
 * binarised mask.  anchor = 0 is the caller's "off": it makes none of the three launches and returns the plain chain.
 * Not handled: anchoring inside the occlusion-aware and the several-keys forms (an occluded block would be matched against the
 * occluder); a subject whose look changes away from the key (turning, relighting beyond what `smooth` refuses) gets e ~ 0 there and
 * drifts as before; re-anchoring every n-th frame only.  (Anchoring inside the single-key occlusion-aware form is the section
 * behind this one, lp_prop_anchor_match_gated; anchoring inside the several-keys form the one behind that.)
 * Launch (csrc/propagate_kernel.hip): lp_prop_anchor_match fuses the warp and the match, K never goes to memory.  A block of 256
 * lanes per 32 x 32 pixels, that is 4 x 4 level-0 blocks: K of the tile and its halo of 4 (40 x 40 bytes, ANDed with the per-byte
 * mask beside it) goes to LDS once, gathered through P_t, which is read as 16-byte vectors when width % 4 == 0 and the planes are
 * 16-byte aligned; the clamped target patch, (40 + 2 anchor)^2 <= 54^2 bytes, next to it.  Each wave takes four windows; the
 * (2 anchor + 1)^2 <= 225 candidates are spread over its lanes in up to four passes, v_alignbyte_b32 cuts the four target pixels
 * out of two patch dwords, v_sad_u8 adds the four absolute differences, the minimum of the key is taken wave-wide and the
 * sub-pixel term from the winner's neighbours as lp_prop_match does it.  A tile without a mask pixel leaves after staging.  One job.
 * LP_E_INVALID: a null pointer, a side outside its range, anchor outside 1..LP_PROP_MAX_SEARCH, smooth outside
 * 0..LP_PROP_MAX_SMOOTH, vec or valid aliasing an input or one another.  All checked before any HIP call.                          */
typedef struct lp_prop_anchor_desc {
    int32_t height, width, anchor, smooth;        /* anchor 1..LP_PROP_MAX_SEARCH, smooth 0..LP_PROP_MAX_SMOOTH             */
    const int32_t* pos;                           /* P_t [height, width, 2], as lp_prop_advance wrote it                    */
    const uint8_t* tgt;                           /* Yt: level 0 of frame t's luma pyramid [height, width]                  */
    const uint8_t* key;                           /* Yk: level 0 of the key frame's luma pyramid                            */
    const uint8_t* mask;                          /* m: level 0 of the pyramid lp_prop_advance wrote                        */
    int32_t*       vec;                           /* out, [gh, gw, 2], the raw correction field                             */
    int32_t*       valid;                         /* out, [gh, gw], 0 / 1: the inputs of lp_prop_fill                       */
} lp_prop_anchor_desc;
LP_API int lp_prop_anchor_match(const lp_prop_anchor_desc* desc, void* stream);

/* ---- Video mask propagate, anchored and occlusion-aware (beyond the reference) -------------------------------------------------------
 * The two single-key refinements above each fail where the other works.  The occlusion-aware form tests against the key frame through
 * positions that have drifted, so on sub-pixel motion drift reads as occlusion and the chain collapses; the anchored form pulls the
 * blocks under an occluder onto the occluder.  This form has both: the anchored re-match with an occlusion gate in the same pass, and
 * the occlusion-aware form's test and split on the corrected positions.  A step is the single-key step with six launches behind it
 * (the existing entries keep their meaning and their bits), 2 levels + 6 in all:
 *   lp_prop_match / lp_prop_fill per level -> lp_prop_advance (out, mask_pyramid to scratch: P_t, c, m = c >= 128)
 *     -> lp_prop_anchor_match_gated -> lp_prop_fill -> lp_prop_advance (vec = e, pos_src = P_t, key bits: P'_t, c', m' = c' >= 128)
 *     -> lp_prop_visible (on P'_t, Yt, Yk, m') -> lp_prop_occlude (on c' and those flags: mask, hidden, next step's bit pyramid).
 * All of it is integer arithmetic.
 * lp_prop_anchor_match_gated does, per level-0 block, exactly what lp_prop_anchor_match does: the same K(y, x) = (bil(Yk, P_t) + 128)
 * >> 8, window and validity (LP_PROP_MIN_PIXELS), candidates, key order, clamping of target coordinates and sub-pixel step.  Then,
 * for a live block with whole-pixel winner (oy, ox), the one the key order chose before the sub-pixel step:
 *   M the mask pixels (m = 1) of the block's window, n = |M|;  d(y, x) = Yt(clamp(y + oy), clamp(x + ox)) - K(y, x);  D = sum_M d;
 *   mu = floor((2 D + n) / (2 n)), the mathematical floor, clamped to +-LP_PROP_VIS_MAX_BIAS;  R = sum_M |d - mu|;
 *   the block is gated iff R > occlusion * n.
 * This is lp_prop_visible's statistic, taken at the alignment the match found, so drift of up to `anchor` pixels is not taken for an
 * occluder.  gated [gh, gw] is 0 / 1, 0 for a block that is not live; valid = live and not gated; vec is lp_prop_anchor_match's
 * vector where valid and 0 elsewhere.  lp_prop_fill gives a gated block the correction of its visible neighbours.  Hence, bit for
 * bit: where gated = 0, vec and valid are lp_prop_anchor_match's; where gated = 1, valid = 0 and vec = 0.
 * The final visibility test is the existing one on the corrected positions; mask, hidden and the bits that weight the next step's
 * match come from lp_prop_occlude, as in the occlusion-aware form.  The key frame returns its binarised mask and a zero hidden;
 * nothing is remembered between frames but the positions.
 * What follows from the rule, bit for bit: a clip of equal frames, and a noise-free whole-pixel shift that the plain chain tracks
 * exactly, return the plain chain's bits and a zero hidden; an empty mask gives 0 and 0; one frame gives the binarised mask; where
 * no block is gated and no final flag fires, mask is the anchored form's and hidden is 0.  anchor = 0 is the caller's "off" for the
 * re-match (the occlusion-aware form, its launches only), occlusion = 0 for the tests (the anchored form and zeros, its launches
 * only), both 0 the plain chain and zeros.
 * Not handled: a subject hidden entirely; what leaves the picture; occlusion edges finer than a block; several keys; a subject
 * whose look changes away from the key.
 * Launch (csrc/propagate_kernel.hip): lp_prop_anchor_match's kernel with a compile-time tail on its window loop.  Behind the
 * wave-wide minimum every lane knows the winner; the window is 16 rows x 4 dwords, the 64 lanes of the wave: each lane cuts its
 * target dword for the winner out of the patch in LDS (v_alignbyte_b32), unpacks four bytes against K under the per-byte mask, D is
 * reduced across the wave, then mu, then R.  LDS as lp_prop_anchor_match has it.  One lane per block writes.  A tile without a mask
 * pixel leaves after staging and writes 0 / 0 / 0.  One job.
 * LP_E_INVALID: a null descriptor or pointer, a side outside 1..LP_VMASK_MAX_SIDE, anchor outside 1..LP_PROP_MAX_SEARCH, smooth
 * outside 0..LP_PROP_MAX_SMOOTH, occlusion outside 1..255, reserved0 != 0, any output aliasing an input or another output.  All
 * checked before any HIP call.                                                                                                     */
typedef struct lp_prop_anchor_gated_desc {
    int32_t height, width, anchor, smooth;        /* anchor 1..LP_PROP_MAX_SEARCH, smooth 0..LP_PROP_MAX_SMOOTH             */
    int32_t occlusion, reserved0;                 /* occlusion 1..255 grey levels; reserved0 must be 0                      */
    const int32_t* pos;                           /* P_t [height, width, 2], as lp_prop_advance wrote it                    */
    const uint8_t* tgt;                           /* Yt: level 0 of frame t's luma pyramid [height, width]                  */
    const uint8_t* key;                           /* Yk: level 0 of the key frame's luma pyramid                            */
    const uint8_t* mask;                          /* m: level 0 of the pyramid lp_prop_advance wrote                        */
    int32_t*       vec;                           /* out, [gh, gw, 2], the raw correction field, 0 where gated              */
    int32_t*       valid;                         /* out, [gh, gw], 0 / 1: the inputs of lp_prop_fill                       */
    int32_t*       gated;                         /* out, [gh, gw], 0 / 1: a live block that does not look like the key     */
} lp_prop_anchor_gated_desc;
LP_API int lp_prop_anchor_match_gated(const lp_prop_anchor_gated_desc* desc, void* stream);

/* ---- Video mask propagate from several keys, anchored (beyond the reference) ----------------------------------------------------------
 * Between two keys the merge pins the mask to each painting, but half way through a long gap both chains have fallen behind the
 * subject by the drift the anchored section describes.  The rule of this form is the several-keys rule with one change: each chain
 * is the anchored chain of its key (the anchored section's steps 1 to 5, the key frame of the chain as Yk); the plan of the chains,
 * what a key frame and a frame outside the keys return, and the merge are unchanged.  K = 1 is the anchored single-key form bit for
 * bit; anchor = 0 is the caller's "off": the several-keys form, its launches only.  A still video with the same mask on every key
 * returns that binarised mask; empty stays exactly 0 and full exactly 1.0.
 * No new entry: the batched re-match is lp_prop_match_batch with reserved0 = LP_PROP_MATCH_WARPED_KEY, since a match job and an anchor
 * job are the same six pointers.  reserved0 = 0 keeps the meaning and the bits it had; any other value but the gated form's below
 * is LP_E_INVALID.  With LP_PROP_MATCH_WARPED_KEY, per job: src is the key frame's luma pyramid and tgt the frame's (level 0 of each
 * is read), mask the pyramid whose level 0 is m, parent the positions P_t int32 [height, width, 2], required whatever `levels` is;
 * level must be 0; search is the anchor, 1..LP_PROP_MAX_SEARCH; vec and valid alias no input and not each other.  The result is
 * exactly lp_prop_anchor_match's for that job: lp_prop_anchor_match and lp_prop_anchor_match_gated are one-job launches of the same
 * kernel, which takes its job from a table on blockIdx.z (32 x 56 bytes by value in its arguments, a `wide` bit per job).
 * A step of a group of up to LP_PROP_MAX_JOBS chains is 2 L + 4 launches:
 *   lp_prop_match_batch / lp_prop_fill_batch per level -> lp_prop_advance_batch (P_t, m to per-chain scratch)
 *     -> lp_prop_match_batch (warped key) -> lp_prop_fill_batch -> lp_prop_advance_batch (vec = e, pos_src = P_t).
 * Not handled here: anchoring inside the several-keys occlusion-aware form -- a gated batch needs a third output and `occlusion`,
 * which this job does not hold; what the anchored section lists.  (The section behind this one is that form: its batch goes
 * without the third output and carries `occlusion` in reserved0, LP_PROP_MATCH_GATED.)
 * LP_E_INVALID in the warped form: level != 0, search outside 1..LP_PROP_MAX_SEARCH, a null pointer in any job (parent included),
 * vec or valid aliasing an input or one another, next to every range lp_prop_match_batch checks.  All checked before any HIP call.
 * The gated form, reserved0 = LP_PROP_MATCH_GATED(occlusion) = LP_PROP_MATCH_WARPED_KEY | (occlusion << 8): occlusion 1..255 in bits
 * 8..15, bits 1..7 and 16..31 zero.  reserved0 = LP_PROP_MATCH_WARPED_KEY, occlusion bits 0, stays the ungated form with the bits it
 * had.  A launch is all gated or all ungated, with one occlusion.  The job is the same six pointers and every check of the warped
 * form holds.  There is no `gated` plane: the kernel writes that plane only where its pointer is non-null, and a batch job has none.
 * Per job, vec and valid are exactly what lp_prop_anchor_match_gated writes for that job: valid = live and not gated, vec = 0 where
 * gated.  The two single entries and the ungated batch return the bits they returned.                                                */

/* ---- Video mask propagate from several keys, anchored and occlusion-aware (beyond the reference) --------------------------------------
 * The last of the eight combinations of the three refinements: several painted keys, every chain anchored, every chain
 * occlusion-aware.  It is for a long clip whose subject moves a fraction of a pixel per frame while something passes in front, with a
 * second key painted behind the occluder: the several-keys occlusion-aware form takes the drift for occlusion there, and the
 * several-keys anchored form pulls the blocks under the occluder onto it and reports no hidden part.
 * The rule is the several-keys occlusion-aware section with one change: every chain is the anchored occlusion-aware chain of its own
 * key, the steps of the "anchored and occlusion-aware" section with Yk the chain's key frame's luma.  For chain X arriving at frame t:
 *   match / fill per level -> advance (P_t, c and m = c >= 128, to per-chain scratch)
 *     -> the gated anchor match on (P_t, Yt, Yk, m) -> fill
 *     -> advance with vec = e, pos_src = P_t and the key bits: P'_t and the code c_X
 *     -> visible on (P'_t, Yt, Yk, c_X >= 128): the flags f_X
 *     -> occlude: c'_X, hidden_X = (c_X - c'_X) / 256, the bits that weight the next step's match, and N_X(t).
 * Everything else is the several-keys occlusion-aware section unchanged, with these c_X, c'_X, f_X and N_X: the plan of the chains,
 * what a key frame and a frame outside the keys return, the lost rule (LP_PROP_MIN_PIXELS, sticky, never for a key with fewer than 16
 * bits) and lp_prop_merge_visible.
 * What follows from the rule, bit for bit: K = 1 is the anchored occlusion-aware single-key form, both outputs; anchor = 0 is the
 * several-keys occlusion-aware form with its launches only; occlusion = 0 is the several-keys anchored form and a zero hidden, with
 * its launches only; both 0 the several-keys form and zeros; a still video with the same mask on every key returns that binarised
 * mask and a zero hidden; empty keys everywhere give 0 and 0; mask + hidden is a multiple of 1 / 256 everywhere; every key frame
 * returns its painting and a zero hidden; a frame outside the keys is the single-key anchored occlusion-aware chain of the nearest
 * key.
 * No new entry.  A step of a group of up to LP_PROP_MAX_JOBS chains is 2 L + 6 launches:
 *   lp_prop_match_batch / lp_prop_fill_batch per level -> lp_prop_advance_batch (P_t, m to per-chain scratch)
 *     -> lp_prop_match_batch (LP_PROP_MATCH_GATED(occlusion)) -> lp_prop_fill_batch -> lp_prop_advance_batch (vec = e, pos_src = P_t)
 *     -> lp_prop_visible_batch -> lp_prop_occlude_batch (mask, hidden, the next step's bit pyramid, the count).
 * Not handled: following a subject through a full occlusion without a second key; what leaves the picture; occlusion edges finer
 * than a block; a subject whose look changes away from its key.  Lost chains are not stopped early.                                  */

/* ---- Video temporal fill (beyond the reference) -------------------------------------------------------------------------------------
 * What lies under the mask of a video frame is, in most clips, plain background a few frames earlier or later: a subject moves
 * across it, or the camera pans past.  These entries borrow it from there, in front of the spatial fill (lp_mask_fill) and the
 * encode:  mask chain -> temporal fill -> (remaining mask) lp_mask_fill -> encode / Detailer crops.  The motion of the background
 * is the block field of the propagate section, weighted by the known pixels (the mask's complement) and continued across the hole
 * by its fill; an origin (frame, position) is carried along it frame by frame in both directions, and the picture is sampled once,
 * at the origin.  Integer arithmetic decides everything except that sample.  Everything stays on the device.
 *   limits    sides 1..LP_VMASK_MAX_SIDE; channels 1..LP_DETAIL_MAX_CHANNELS; frames F <= 65535; levels, search and smooth as in the
 *             propagate section; reach 0..LP_TFILL_MAX_REACH, 0 meaning the whole clip.  Positions are (y, x) pairs of int32 in
 *             1/16 pixel; `>>` is the arithmetic shift.
 * 1 known     m = mask >= 0.5 (a NaN gives 0, as lp_prop_key_mask binarises), known = 1 - m.  Every frame gets the pyramid of its
 *             known bits: the footprints, the OR rule and the byte layout of the propagate section's stage 2
 *             (lp_prop_pyramid_ws_bytes(1, ...) is a frame's stride).  lp_tfill_known builds them for all frames, a mask of one
 *             frame serving every frame, and unless the pointers are null the planes the carry starts from:
 *             source[t] = t on a known pixel and -1 under the mask, remaining[t] = 0.0 and 1.0.  A call for a part of the clip
 *             names its first frame in frame0, 0..65535 - frames.
 * 2 fields    For a direction d in {+1, -1} and a frame t whose donor t - d is a frame of the clip, the field of the step is the
 *             level-0 final field of the propagate section's stage 3 (match, fill and median, levels L - 1 down to 0) with
 *             src = the luma pyramid of frame t, tgt = the luma pyramid of frame t - d, mask = the known pyramid of frame t;
 *             V(y, x) is that section's "per pixel" interpolation, and pixel (y, x) of t lies at q = (16 y + Vy, 16 x + Vx) in the
 *             donor.  A field depends on the two frames and the mask of t only, never on what was carried, so the 2 (F - 1) fields
 *             of a clip are independent jobs of lp_prop_match_batch / lp_prop_fill_batch, LP_PROP_MAX_JOBS to a launch.
 * 3 carry     (lp_tfill_carry, one step of one direction) The state of a frame is per pixel an origin (f, P), a frame and a position
 *             in it, or none.  A known pixel (y, x) of t has the origin (t, (16 y, 16 x)).  A masked pixel: if q is outside
 *             0..16 (n - 1) on either axis it has none from this direction; otherwise i = (q + 8) >> 4 per axis, r = q - 16 i, and
 *             if the donor's pixel i has an origin (f, P) with |t - f| <= reach the pixel's origin is (f, P + r), else none.  The
 *             first frame of a direction has only its known pixels.  The donor's state under its known pixels is implicit (its
 *             known bits are read, not a stored plane), so the state planes org [height, width] (f, or -1 for none) and pos
 *             [height, width, 2] are written and read under the mask only; null state planes of the donor say it has none there.
 * 4 choice    The forward pass (d = +1, t ascending, nearer = 0) runs first and writes every masked pixel for which it has an
 *             origin.  The backward pass (d = -1, t descending, nearer = 1) writes a pixel only where source[t] is -1 or |t - f| is
 *             strictly smaller than |t - source[t]|: a tie stays with the past.  A written pixel gets source[t] = f,
 *             remaining[t] = 0.0 and the sample.  So source[t] ends as f, as t itself on a known pixel, or as -1 where neither pass
 *             found an origin, and remaining = 1.0 exactly where m = 1 and source = -1.
 *   sample    of images[f] at P clamped to 0..16 (n - 1) per axis: i = P >> 4, fr = P & 15, i1 = min(i + 1, n - 1); per channel
 *             row(a, b) = fx == 0 ? 16 a : (16 - fx) a + fx b, value = (fy == 0 ? 16 top : (16 - fy) top + fy bot) * (1 / 256), in
 *             fp32, every product and sum rounded on its own (no FMA).  A tap with weight 0 is not read, so a non-finite
 *             neighbour cannot leak.  Image values pass through as fp32, neither clamped nor coded.  `filled` starts as a copy of
 *             `images` (the caller's), so a pixel with source in {t, -1} keeps images[t] bit for bit.
 * What follows from the rule: one frame, an empty mask or a full mask returns the images unchanged; a subject that does not move
 * against the background is left entirely in `remaining`; under noise-free whole-pixel motion the borrowed pixels equal the true
 * background bit for bit; nothing outside the mask ever changes; the same bits on every run and for every chunking of the fields.
 * Launches (csrc/temporal_fill_kernel.hip): lp_tfill_known 1 + (levels - 1) for all its frames; lp_tfill_carry one, a block per
 * 32 x 32 tile that leaves after reading its known bytes when all are 1.  A call is the two pyramids, 2 L launches per
 * LP_PROP_MAX_JOBS fields and 2 (F - 1) carries; only the carries depend on one another.
 * LP_E_INVALID: a null pointer (except source and remaining of lp_tfill_known, and the donor's state planes, both or neither); a
 * side, levels, channels or reach outside its range; frames <= 0 (lp_tfill_carry: frames < 2); mask_frames neither 1 nor frames;
 * frame0 < 0; frame or donor outside the clip or not neighbours; nearer not 0 / 1; an output plane that is an input or another
 * output.  LP_E_UNSUPPORTED: frames or frame0 + frames > 65535.  All checked before any HIP call.                                  */
#define LP_TFILL_MAX_REACH  65535

typedef struct lp_tfill_known_desc {
    int32_t frames, height, width, levels;
    int32_t mask_frames, frame0;                  /* 1: one mask plane for every frame, else == frames; frame0: see source  */
    const float* mask;                            /* [mask_frames, height, width] fp32                                      */
    uint8_t*     pyramid;                         /* out, lp_prop_pyramid_ws_bytes(frames, height, width, levels) bytes      */
    int32_t*     source;                          /* out or null, [frames, height, width]; plane f is frame t = frame0 + f  */
    float*       remaining;                       /* out or null, [frames, height, width]                                   */
} lp_tfill_known_desc;
LP_API int lp_tfill_known(const lp_tfill_known_desc* desc, void* stream);

typedef struct lp_tfill_carry_desc {
    int32_t frames, height, width, channels;
    int32_t frame, donor;                         /* t and t - d, neighbours inside the clip                                */
    int32_t reach, nearer;                        /* nearer 0: write wherever an origin is found; 1: only where it is nearer */
    const int32_t* vec;                           /* the step's level-0 final field [gh, gw, 2]                             */
    const uint8_t* known;                         /* frame t's known bits [height, width] (level 0 of its pyramid)          */
    const uint8_t* donor_known;                   /* the donor's                                                            */
    const int32_t* org_src;                       /* the donor's state [height, width]; null with pos_src: none             */
    const int32_t* pos_src;                       /* [height, width, 2]                                                     */
    int32_t*       org_dst;                       /* out, frame t's state, written under its mask only                      */
    int32_t*       pos_dst;
    const float*   images;                        /* [frames, height, width, channels] fp32                                 */
    float*         filled;                        /* in / out, [frames, height, width, channels]: frame t is written        */
    int32_t*       source;                        /* in / out, [frames, height, width]: frame t is read (nearer) and written */
    float*         remaining;                     /* in / out, [frames, height, width]: frame t is written                  */
} lp_tfill_carry_desc;
LP_API int lp_tfill_carry(const lp_tfill_carry_desc* desc, void* stream);

/* Checked temporal fill.  The fill above believes the one-layer background field everywhere: when something other than the masked
 * subject moves through the hole it borrows the wrong picture, and a wrong known pixel is worse than one left in `remaining`.
 * Here the two directions are witnesses of one another: where both have an origin for a pixel and their samples disagree over a
 * block, the block is left to the sampler.  Stages 1 to 4 stay word for word; the forward pass is lp_tfill_carry with nearer = 0,
 * unchanged.  After it a masked pixel p of frame t with source[t](p) = f_A >= 0 has witness A, and S_A = filled[t](p) is its
 * sample.  The backward pass is one launch of lp_tfill_carry_pair per step t <- t + 1 (donor = frame + 1), t = F - 2 .. 0:
 * 1 witness B   Stage 3 gives B, the backward origin (f_B, P_B), reach applied as there; S_B is its stage-"sample" value.  The
 *               state written for the next step (org_dst, pos_dst) is exactly what lp_tfill_carry writes: a dispute never alters
 *               what is carried.
 * 2 luma        both = masked and has A and has B.  Y_A, Y_B are the propagate section's 8-bit luma codes of S_A and S_B (stage
 *               "1 luma" there: a NaN gives 0, +inf 255; channels 1 or 2 take channel 0);  d = Y_B - Y_A.
 * 3 block flag  per block of LP_PROP_BLOCK x LP_PROP_BLOCK pixels, aligned to the plane's origin and cut at its edges (no halo):
 *               M = the block's `both` pixels, n = |M|.  n < LP_PROP_MIN_PIXELS: the flag is 0, for lack of evidence.  Else
 *               D = sum over M of d; mu = floor((2 D + n) / (2 n)), the mathematical floor, clamped to +-LP_PROP_VIS_MAX_BIAS (a
 *               brightness bias between the two frames is forgiven); R = sum over M of |d - mu|; the flag is 1 (disputed) iff
 *               R > agree * n, with agree in 1..255 the mean residual in grey levels.  The arithmetic of lp_prop_visible, on
 *               integers: the order of the sums cannot matter.
 * 4 per masked pixel
 *               disputed (both and flag 1): filled = images[t], source = -2 (LP_TFILL_DISPUTED), remaining = 1.0, witnesses = 0;
 *               both and flag 0: stage 4's choice, B is written iff |t - f_B| < |t - f_A| (a tie stays with the past);
 *                                witnesses = 2 when n >= LP_PROP_MIN_PIXELS, else 1;
 *               only A: left as it is, witnesses = 1;     only B: B is written as in stage 4, witnesses = 1;
 *               neither: remaining = 1.0, witnesses = 0.  A known pixel has witnesses = 0.
 *               witnesses int32 [frames, height, width]: the launch writes every pixel of plane t, known ones included.
 * Frame F - 1 has no backward step, so A alone counts there: witnesses = 1 where it is masked and source >= 0, else 0 (the
 * caller's, from `source`, on the device).
 * What follows from the rule: wherever source != -2 the outputs filled, remaining and source carry the bits of the plain fill on
 * the same arguments; wherever source == -2 the plain fill had source >= 0 and the checked one returns images; remaining = 1.0
 * exactly where m = 1 and source < 0; the same bits on every run and for every chunking of the fields.
 * Launch (csrc/temporal_fill_kernel.hip): the carry's geometry, a block of 1024 lanes per 32 x 32 tile -- exactly 16 aligned
 * blocks of 8 x 8, so no sum crosses a tile -- that leaves after reading its known bytes (and writing witnesses = 0) when all are
 * 1.  Else two integer reductions per block in LDS, n and D packed in one word, then R, a barrier between them; every lane of the
 * tile reaches both.  The B sample is gathered wherever B exists, not only where it is nearer.  No scratch, no global atomics.
 * LP_E_INVALID: as lp_tfill_carry, and donor != frame + 1, agree outside 1..255, a null witnesses, witnesses aliasing any other
 * plane.  LP_E_UNSUPPORTED: frames > 65535.  All checked before any HIP call.                                                    */
#define LP_TFILL_DISPUTED   (-2)

typedef struct lp_tfill_carry_pair_desc {
    int32_t frames, height, width, channels;
    int32_t frame, donor;                         /* t and t + 1                                                            */
    int32_t reach, agree;                         /* agree 1..255                                                           */
    const int32_t* vec;                           /* as in lp_tfill_carry_desc                                              */
    const uint8_t* known;
    const uint8_t* donor_known;
    const int32_t* org_src;
    const int32_t* pos_src;
    int32_t*       org_dst;
    int32_t*       pos_dst;
    const float*   images;
    float*         filled;                        /* in / out: frame t holds S_A where A exists; only the own pixel is touched */
    int32_t*       source;                        /* in / out: frame t holds f_A, -1 or t                                   */
    float*         remaining;                     /* in / out: frame t is written                                           */
    int32_t*       witnesses;                     /* out, [frames, height, width]: frame t is written, every pixel          */
} lp_tfill_carry_pair_desc;
LP_API int lp_tfill_carry_pair(const lp_tfill_carry_pair_desc* desc, void* stream);

/* ---- Video temporal smooth (beyond the reference) -----------------------------------------------------------------------------------
 * The sampler invents what lies under the mask frame by frame, so texture that should be one piece of background boils from frame
 * to frame.  This entry follows the picture's motion from every masked pixel a few frames into the past and the future, looks at
 * what the sampler put at the same scene point there, and pulls the pixel towards the weighted mean of what agrees with it:
 *   decode / stitch -> temporal smooth -> multiband blend -> grain match.  Grain is synthesized afterwards, which is why smoothing
 * it away here is wanted.  Integer arithmetic decides where every sample is taken and whether it counts; the sums are fp32 in a
 * fixed order.  Everything stays on the device.
 *   limits    sides, channels, frames, levels, search and smooth as in the temporal fill section; radius R in
 *             1..LP_TSMOOTH_MAX_RADIUS; tolerance 0..255 grey levels.  Positions are (y, x) pairs of int32 in 1/16 pixel; `>>` is
 *             the arithmetic shift.
 *   mask      m = mask >= 0.5 (a NaN gives 0: known), exactly as lp_tfill_known binarises; known = 1 - m.
 *   fields    The field of frame u towards its neighbour v = u +- 1 is stage 2 of the temporal fill section, word for word: the
 *             level-0 final field of the propagate section with src = the luma pyramid of u, tgt = that of v.  With motion
 *             "background" the weights are the known pyramid of u: exactly the fields the temporal fill computes.  With motion
 *             "picture" the weights are the pyramid of an all-known plane, every pixel weighs in: for an inpainted subject that
 *             moves on its own.  V_{u->v}(i) is that section's "per pixel" interpolation at the integer pixel i.  The motion is the
 *             caller's choice of fields; the entry takes the fields.
 *   walk      per masked pixel (y, x) of frame t and per direction d in {-1, +1}.  p_0 = (16 y, 16 x).  For k = 1..R:
 *             u = t + (k - 1) d, v = t + k d.  The chain ends if v is outside the clip.  Otherwise i = (p_{k-1} + 8) >> 4 per axis
 *             and q = p_{k-1} + V_{u->v}(i); the chain ends if q is outside 0..16 (n - 1) on either axis.  Otherwise s_k is the
 *             temporal fill section's `sample` of images[v] at q: the same taps, the same fp32 order, a tap with weight 0 is not
 *             read.  The sample is accepted iff max over channels of |code(s_k[c]) - code(x[c])| <= tolerance, with
 *             x = images[t, y, x] and code the project's 8-bit code: clamp to 0..1 with NaN -> 0, then (int)(v * 255.0f + 0.5f),
 *             product and sum rounded on their own.  The chain ends at the first sample that is not accepted; otherwise p_k = q.
 *             A chain that has ended contributes nothing further in its direction.
 *   result    under the mask.  Integer weights w_k = C(2R, R + k).  acc = 0; then, in the order of the walk (k = -1, -2, .., -R,
 *             then +1, .., +R: past before future, nearer before farther), for every accepted sample, per channel
 *             acc = acc + w_k * (s_k - x), the difference, the product and the sum each rounded to fp32 on its own (no FMA).
 *             W = w_0 + the sum of the accepted w_k; W <= 65536, exact in fp32.  out = x + acc / W, an IEEE division and a sum,
 *             rounded on their own.  A pixel with no accepted sample keeps x bit for bit.  support (int32) = the number of
 *             accepted samples, 0..2R.
 *   outside   the mask out = images bit for bit and support = -1.
 * What follows from the rule: one frame returns the images; an empty mask returns the images; a clip whose masked area does not
 * change along the field is returned bit for bit (the difference form gives exactly 0); nothing outside the mask ever changes; an
 * object more than `tolerance` away from the pixel is never averaged in; the same bits on every run and for every chunking.
 * Non-finite values behave as fp32 arithmetic gives: a NaN or a negative value has code 0 and +inf code 255, so a non-finite sample
 * can be accepted, and an accepted NaN sample makes that pixel NaN.
 * Not done: a reference value other than the frame's own pixel -- a single outlier frame therefore keeps its value, because every
 * neighbour is rejected; motion boundaries finer than a block; a soft mask edge (the multiband blend follows).
 * Launch (csrc/temporal_smooth_kernel.hip): one for the frames first .. first + count - 1 of the clip, a block per 32 x 32 tile and
 * frame, a lane per pixel; a wave (two rows of a tile) with nothing masked copies its pixels and leaves, elsewhere a known pixel is copied by its lane.  `fwd` row j is the field of frame fwd_first + j towards the next
 * frame, `bwd` row j that of frame bwd_first + j towards the one before, [gh, gw, 2] each; the walks read `fwd` of the frames
 * first .. min(first + count + R - 2, frames - 2) and `bwd` of max(first - R + 1, 1) .. first + count - 1, and the rows given must
 * cover those.  Where a range is empty (one frame) its pointer is not read and may be null.  `known` is level 0 of frame
 * `first`'s known pyramid, the next frame's known_stride bytes on (a frame's pyramid stride, or height * width).  No scratch, no
 * atomics, no LDS.
 * LP_E_INVALID: a null pointer (except an unread field array); frames < 1; a side, channels, radius or tolerance outside its range;
 * first < 0, count < 1 or first + count > frames; field rows that do not cover what is read; known_stride < height * width with
 * count > 1; out or support aliasing an input or one another.  LP_E_UNSUPPORTED: frames > 65535.  All checked before any HIP call. */
#define LP_TSMOOTH_MAX_RADIUS 8

typedef struct lp_tsmooth_desc {
    int32_t frames, height, width, channels;      /* the clip                                                                */
    int32_t first, count;                         /* the frames this launch writes                                           */
    int32_t radius, tolerance;
    int32_t fwd_first, fwd_count;                 /* the frames whose rows `fwd` holds                                       */
    int32_t bwd_first, bwd_count;
    const int32_t* fwd;                           /* [fwd_count, gh, gw, 2] level-0 final fields towards the next frame      */
    const int32_t* bwd;                           /* [bwd_count, gh, gw, 2] towards the frame before                         */
    const uint8_t* known;                         /* frame `first`'s known bits [height, width]                              */
    int64_t        known_stride;                  /* bytes from a frame's known bits to the next frame's                     */
    const float*   images;                        /* [frames, height, width, channels] fp32                                  */
    float*         out;                           /* [frames, height, width, channels]: frames first .. are written, whole   */
    int32_t*       support;                       /* [frames, height, width]: likewise                                       */
} lp_tsmooth_desc;
LP_API int lp_tsmooth(const lp_tsmooth_desc* desc, void* stream);
/* The robust form below (lp_tsmooth_robust) takes a temporal median as the reference value, so that an outlier frame is repaired. */

/* ---- Robust video temporal smooth (beyond the reference) ----------------------------------------------------------------------------
 * lp_tsmooth compares every neighbouring sample with the frame's own pixel, so the one frame in which the sampler invented
 * something else under the mask -- a "pop", the defect a viewer sees first -- keeps its value, and a neighbour of that frame loses
 * its whole chain on that side.  This entry is a second, stricter form beside it: the reference value is the temporal median of
 * the samples along the motion, every sample is compared with that, and a pixel that disagrees with it is overruled when two
 * witnesses stand against it.  It takes the plain smooth's place: decode / stitch -> robust temporal smooth -> multiband blend ->
 * grain match.  Integer arithmetic decides where every sample is taken, which is the reference and what counts; the sums are fp32
 * in a fixed order.  Everything stays on the device.
 *   limits, mask, fields, `sample`, code, the 1/16-pixel positions and the integer weights w_k = C(2R, R + k) are those of the
 *             lp_tsmooth section, word for word.
 *   walk      per masked pixel (y, x) of frame t and per direction d in {-1, +1}.  p_0 = (16 y, 16 x).  For k = 1..R:
 *             u = t + (k - 1) d, v = t + k d.  The chain ends if v is outside the clip.  Otherwise i = (p_{k-1} + 8) >> 4 per axis
 *             and q = p_{k-1} + V_{u->v}(i); the chain ends if q is outside 0..16 (n - 1) on either axis.  Otherwise p_k = q and
 *             the step exists: it gives the sample `sample`(images[v], q).  A chain does NOT end at a sample that is rejected
 *             later: the trajectory depends on the fields only, so a pop frame in between does not cut off the frames behind it.
 *             The order index o is 0 for the own pixel, s_0 = x = images[t, y, x]; k for step k into the past (d = -1); R + k for
 *             step k into the future.  X is the set of the o that exist, n = |X| <= 2R + 1.
 *   luma      Y_o = the propagate section's 8-bit luma of the sample's codes: (77 c0 + 150 c1 + 29 c2 + 128) >> 8 with
 *             c_i = code(s_o[i]) where channels >= 3, else c0 -- the quantity the checked temporal fill compares.
 *   reference if n < 3, j* = 0.  Otherwise X is sorted by the pair (Y_o, o) ascending and j* is the element at 0-based position
 *             (n - 1) >> 1: the lower median, ties broken by the walk's order.  r = s_{j*}, a whole sample with every channel; it
 *             is x itself when j* = 0.
 *   accepted  o in X is accepted iff max over channels of |code(s_o[c]) - code(r[c])| <= tolerance.  a = the number of accepted
 *             o != 0.  LP_TSMOOTH_ROBUST_QUORUM = 2 is a constant of the rule, not a parameter.
 *   result    under the mask, three cases; fp32, the difference, the product, the sum and the division each rounded on its own (no
 *             FMA), the terms in the order of the walk (o = 1, .., R, then R + 1, .., 2R: past before future, nearer before
 *             farther), w of o being w_k of its step k.
 *             1. the own pixel is accepted: acc = sum of w (s_o - x) over the accepted o != 0, W = w_0 + their weights,
 *                out = x + acc / W, and with a = 0 the output keeps x bit for bit.  support = a, replaced = 0.
 *             2. the own pixel is not accepted and a >= LP_TSMOOTH_ROBUST_QUORUM -- two witnesses overrule the pixel, the reference
 *                and at least one more sample: acc = sum of w (s_o - r) over the accepted o not in {0, j*}, W = the weights of the
 *                accepted o != 0 (that of j* among them, w_0 not), out = r + acc / W.  support = a, replaced = 1.
 *             3. the own pixel is not accepted and a < LP_TSMOOTH_ROBUST_QUORUM: out = x bit for bit, support = 0, replaced = 0.
 *             W <= 65536, exact in fp32.
 *   outside   the mask out = images bit for bit, support = -1 and replaced = -1.
 * Non-finite values behave as in the plain rule: a NaN or a negative value has code 0 and +inf code 255, and the fp32 arithmetic
 * is taken as it comes.
 * What follows from the rule (checked on the clips of tests/test_temporal_smooth_host.py): where nothing is rejected under either
 * reference -- a pan with alternating flicker below the tolerance -- out and support are the plain rule's bit for bit and replaced
 * is 0 under the mask.  A pop of one frame (+64/256 under the mask of one frame of a clean pan) is removed: the result is the clean
 * clip bit for bit in every frame for R = 1, 2, 3, replaced == 1 on every masked pixel of that frame and nowhere else, where the
 * plain rule returns the input.  The same pop on two frames in a row is removed for R = 2, 3 and returned bit for bit for R = 1:
 * whatever lasts R frames or fewer under the mask is an outlier and is removed on purpose, whatever lasts longer stays.  A clip of
 * one frame returns the images; a clip of two frames gives the plain rule's bits (n < 3: the reference is the own pixel and a chain
 * has one step); an empty mask returns the images; a still clip is returned bit for bit; nothing outside the mask ever changes; the
 * same bits on every run and for every chunking.
 * Not done: a weighted median; a quorum the caller sets; motion boundaries finer than a block; a soft mask edge.
 * Launch (csrc/temporal_smooth_kernel.hip): as lp_tsmooth's, one for the frames first .. first + count - 1, a block per 32 x 32
 * tile and frame, a lane per pixel, the wave-wide copy where nothing is masked.  A masked pixel walks up to three times -- the
 * positions are integers and come out the same --: for the lumas, packed four to a dword and ranked by counting; to j* for r; and
 * for the acceptance and the sums, four channels at a time.  The fields, `known` and the rows that must be covered are those of
 * lp_tsmooth.  The frames first .. first + count - 1 of out, support and replaced are written whole.  No scratch, no atomics, no
 * LDS.
 * LP_E_INVALID and LP_E_UNSUPPORTED: as lp_tsmooth, with `replaced` not null and out, support and replaced aliasing neither an
 * input nor one another.  All checked before any HIP call. */
#define LP_TSMOOTH_ROBUST_QUORUM 2

typedef struct lp_tsmooth_robust_desc {
    int32_t frames, height, width, channels;      /* lp_tsmooth_desc's fields, in its order                                  */
    int32_t first, count;
    int32_t radius, tolerance;
    int32_t fwd_first, fwd_count;
    int32_t bwd_first, bwd_count;
    const int32_t* fwd;
    const int32_t* bwd;
    const uint8_t* known;
    int64_t        known_stride;
    const float*   images;
    float*         out;
    int32_t*       support;
    int32_t*       replaced;                      /* [frames, height, width]: frames first .. are written, whole             */
} lp_tsmooth_robust_desc;
LP_API int lp_tsmooth_robust(const lp_tsmooth_robust_desc* desc, void* stream);

/* ---- Video shot detect (beyond the reference) ---------------------------------------------------------------------------------------
 * Every temporal link of the video chain (the propagates, the stabilize, the two temporal fills, the temporal smooth) takes a clip
 * as one continuous shot.  Across a hard cut the block matcher still returns a field, and that field means nothing.  These entries
 * give the boundary signal: two integer scores per pair of neighbouring frames and a decision that turns them into a shot index per
 * frame, so that the host can run every link shot by shot.  Integers throughout: the same bits on every run, and the chunking of
 * the frames cannot change a bit, because a score depends on its two frames only.  Everything stays on the device.
 *   limits    level 0..LP_PROP_MAX_LEVELS - 1; search R in 1..LP_SHOT_MAX_SEARCH = 3 ((2R + 1)^2 <= 49 displacements: the lanes of
 *             one wave); frames F in 1..65535; sides of the plane 1..LP_VMASK_MAX_SIDE.
 *   plane     Y_t, the plane of frame t, is level `level` of the 8-bit luma pyramid of the propagate section (stages 1 and 2, built
 *             by lp_prop_luma with levels = level + 1): h x w with N = h w pixels.  clamp(i) holds a coordinate inside the plane.
 *   A[t]      the motion-compensated residual of the pair (t, t + 1), t = 0..F - 2.  Blocks of LP_PROP_BLOCK = 8 are aligned to the
 *             plane's origin and cut at its edges.  For block b with pixel set P and every displacement d = (dy, dx) in [-R, R]^2:
 *             SAD_b(d) = sum over p in P of |Y_t(p) - Y_{t+1}(clamp(p + d))|.  A[t] = sum over b of min over d of SAD_b(d).
 *             A[t] <= 255 * 2^28: an int64.
 *   B[t]      the histogram change of the pair.  h_t[k] = the number of pixels of Y_t with Y >> 2 == k, k = 0..63;
 *             B[t] = sum over k of |h_t[k] - h_{t+1}[k]|.  A pixel that changes its bin counts twice: B[t] <= 2 N.
 *   score     int64 [F - 1, 2]: score[t] = (A[t], B[t]).
 *   decision  threshold 1..255, hist 0..100, ratio 100..10000, window 1..LP_SHOT_MAX_WINDOW = 16.  cut[t] = 1 iff all of
 *               A[t] >= threshold * N                     (the mean residual, in grey levels)
 *               100 * B[t] >= hist * 2 N                  (the share of the pixels that change their bin, in percent)
 *               100 * A[t] >= ratio * A[u]                for every other pair u != t with |u - t| <= window and 0 <= u <= F - 2.
 *             Every product stays below 2^50.  The last condition keeps a flash (two high pairs in a row, neither beats the other),
 *             a run of fast motion and a large object that moves further than the search (its residual is high, its histogram
 *             stays) from being called cuts.  It also makes `window` the shortest shot that can be told apart: two cuts closer
 *             than `window` pairs suppress one another unless one residual is `ratio` percent of the other, and with ratio > 100
 *             two equal residuals inside a window are never cuts; with ratio = 100 both are.
 *   shot      int32 [F]: shot[0] = 0, shot[f] = sum over t < f of cut[t].  F = 1 gives shot = [0]; there is no score.
 * Not done: dissolves, fades and wipes are not detected (no pair of such a transition stands out of its neighbours); the
 * several-key propagates (but the anchored occlusion-aware one, which with its options off is each of them) and the colour match's
 * pooling over neighbouring frames have no shot-aware form.
 * Launches (csrc/shot_kernel.hip).  lp_shot_measure, for the `frames` planes of a chunk: the histograms and the A words are
 * cleared, then one launch for all frames, a 256-lane block per 32 x 32 tile and frame.  The block adds its pixels into per-wave
 * 64-bin histograms in LDS, folded once per block into hist[t] with at most one integer atomic per bin.  If frame t + 1 is in the
 * chunk the tile of t and the (32 + 2R)^2 clamped window of t + 1 are staged in LDS once and the tile's sixteen 8 x 8 blocks are
 * matched, one per wave and round, the displacements over the lanes (v_alignbyte_b32 cuts four pixels out of two dwords, v_sad_u8
 * adds four absolute differences), a wave-wide minimum per block; the tile leaves one 64-bit integer atomic into A[t].  A second,
 * small launch folds hist[t], hist[t + 1] into B[t].  Integer sums: no order changes a bit.  score receives frames - 1 rows, hist
 * (int32 [frames, 64], a workspace that holds the histograms afterwards) frames rows.  Neighbouring chunks share one frame.
 * lp_shot_decide is one block: lanes stride over the pairs, every pair looks at up to 2 window neighbours, the cut bits of 64
 * pairs are one ballot word in LDS, and a scan over the words' counts gives `shot`.  No scratch, no floating point.
 * LP_E_INVALID: a null pointer (score may be null exactly when frames == 1); frames < 1; a side, search, stride (< height * width
 * with frames > 1), n_pixels (1..2^28), threshold, hist, ratio or window outside its range; hist, score and plane, or shot and
 * score, aliasing.  LP_E_UNSUPPORTED: frames > 65535.  All checked before any HIP call. */
#define LP_SHOT_MAX_SEARCH 3
#define LP_SHOT_MAX_WINDOW 16
#define LP_SHOT_BINS       64

typedef struct lp_shot_measure_desc {
    int32_t frames, height, width, search;        /* the chunk's frames; height x width: the plane's own sides               */
    const uint8_t* plane;                         /* frame 0's plane [height, width] (its level's address in the pyramid)    */
    int64_t        stride;                        /* bytes from a frame's plane to the next frame's                          */
    int32_t*       hist;                          /* out, [frames, LP_SHOT_BINS]                                             */
    int64_t*       score;                         /* out, [frames - 1, 2]: (A, B) per pair                                   */
} lp_shot_measure_desc;
LP_API int lp_shot_measure(const lp_shot_measure_desc* desc, void* stream);

typedef struct lp_shot_decide_desc {
    int32_t frames, threshold, hist, ratio;
    int32_t window, reserved0;
    int64_t        n_pixels;                      /* N = the plane's height * width                                          */
    const int64_t* score;                         /* [frames - 1, 2]                                                         */
    int32_t*       shot;                          /* out, [frames]                                                           */
} lp_shot_decide_desc;
LP_API int lp_shot_decide(const lp_shot_decide_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LANPAINT_HIP_H */
