/*
 * fleetplace.h -- C ABI of the MI355X-native FleetFlow placement planner
 * (libfleetplace.so, HIP/gfx950).  This is the drop-in boundary for the
 * reference's plan path.
 *
 * Reference interfaces this ABI replaces (paths relative to chronista-club/fleetflow):
 *   fp_legacy_order   <- fn order_by_dependencies(&[String], &Flow) -> Vec<String>
 *                        crates/fleetflow-container/src/engine.rs:64-85
 *                        (names -> u32 ids in stage order are mapped by the caller;
 *                         strings never cross this ABI)
 *   fp_levelize       <- new: Kahn start levels generalising engine.rs:67-85
 *                        (replaces the call at engine.rs:157 when levels are wanted)
 *   fp_place          <- `stages[stage].servers.first()` with "local" fallback
 *                        crates/fleetflow-controlplane/src/handlers/deploy.rs:386-398
 *                        (N = 1, unconstrained capacity reproduces it exactly)
 *   fp_place_batch    <- new: what-if scenarios, one plan per scenario + packed cost
 *   fp_place_policy   <- new: fp_place under the tenant PlacementPolicy's strategy and preferred labels
 *                        crates/fleetflow-controlplane/src/model.rs:56-95 (schema nothing reads upstream)
 *   fp_place_policy_spread <- new: the same under the policy's SpreadConstraint{topology_key, max_skew}
 *                        crates/fleetflow-controlplane/src/model.rs:56-63
 *   fp_place_policy_fallback <- new: the same under the policy's FallbackPolicy{relax_order, max_hops}
 *                        crates/fleetflow-controlplane/src/model.rs:47-54
 *   fp_place_policy_quota <- new: the same under the policy's ResourceQuota{max_services_per_stage, cpu_cores,
 *                        memory_gb}  crates/fleetflow-controlplane/src/model.rs:38-45
 *   fp_feasibility    <- new: stage-2 containers x nodes feasibility/score sweep
 *   fp_dev_feasibility_batch <- new: the same sweep over many what-if scenarios
 *   fp_explain        <- new: per-cause diagnosis of unplaced containers (which 2.3 predicate fails where)
 *   fp_explain_batch  <- new: the same as one cause histogram per what-if scenario
 *   fp_drain_sweep    <- new: evacuate each server, or each topology domain, from a live plan: the `drain`
 *                        scheduling state, under which existing placements leave as well (`cordon` only
 *                        stops new ones)  crates/fleetflow-controlplane/src/model.rs:435-442
 *   fp_drain_sweep_policy <- new: the same sweep with every move held to the policy's SpreadConstraint and
 *                        FallbackPolicy, on counts that leave the candidate's own servers out (model.rs:47-63;
 *                        the ResourceQuota of model.rs:38-45 has nothing to test: a move releases and retakes
 *                        the same request)
 *   fp_shrink_sweep   <- new: the servers a live plan can give back when they are tried in a given order, for
 *                        many orders at once: the `drain` state applied server after server, each release on
 *                        the state the earlier ones left  crates/fleetflow-controlplane/src/model.rs:435-442
 *   fp_shrink_sweep_policy <- new: the same sweep with every move held to the policy's SpreadConstraint and
 *                        FallbackPolicy (model.rs:47-63) and every release to the bound rule: a server is given
 *                        back only if that leaves the skew within max_skew or no larger than it was
 *   fp_rebalance_sweep <- new: the seats a live plan gives up, one after the other in a given victim order, to
 *                        bring the policy's SpreadConstraint back within max_skew (the descheduler to the
 *                        scheduler's PodTopologySpread), for many orders at once; each seat is re-placed under
 *                        the constraint and the FallbackPolicy
 *                        crates/fleetflow-controlplane/src/model.rs:56-63 and :435-442
 *   fp_grow_sweep     <- new: the new servers of each template (a plan string's size,
 *                        crates/fleetflow-cloud-sakura/src/provider.rs:15-30, with the ServerLabels /
 *                        ServerCapacity a new server would carry, crates/fleetflow-controlplane/src/model.rs:399-419)
 *                        that a plan's unplaced containers need
 *   fp_replan         <- new: the next plan of a stage that already runs: a container stays on its server while
 *                        it still fits there and only the others are placed.  `cordon` "stops new placements,
 *                        existing placements continue" (crates/fleetflow-controlplane/src/model.rs:435-442);
 *                        ServerAllocated is committed and released per placement (model.rs:421-427)
 *   fp_replan_policy  <- new: the same under the policy's SpreadConstraint, FallbackPolicy and ResourceQuota:
 *                        the seats are counted and charged, never tested or evicted; only new and moved
 *                        placements are held to the guarantees (model.rs:38-63)
 *
 * Conventions
 *   - All buffers are caller-owned; no allocation crosses the ABI.
 *   - fp_* take HOST pointers and are synchronous: on error nothing is written.
 *   - fp_dev_* take DEVICE (HBM) pointers of the context's device and are
 *     asynchronous on the context's stream.  The one deviation: relax_mask of
 *     fp_dev_drain_sweep_policy is a HOST array, read during the call like a scalar.  Kernel-side errors of fp_dev_* calls
 *     (FP_ECORRUPT input, FP_EDEVICE from the placement pipeline's deadlock guard) are
 *     sticky: the first one raised is kept until fp_ctx_sync() reports it and clears it.
 *     A host-pointer call reports only the errors of its own kernels (it has its own error
 *     word): a pending asynchronous error neither fails it nor is cleared by it.
 *     fp_dev_* calls read nothing back: every data-dependent choice (key range, sort path,
 *     bucket thresholds, level count, a corrupt CSR) is made on the device, so a caller can
 *     queue call i+1 behind call i's collectives without a host stall.  The exceptions: the
 *     first call of a shape larger than any before it grows the context's workspace (one
 *     stream synchronisation), and FP_OPT_LEVELIZE_SYNC = 1 (the level-synchronous
 *     levelizer) reads its frontier size back once per 64 levels.
 *   - fp_ctx_set_stream first waits for the context's last fp_dev_* call (an event
 *     recorded on the old stream; the workspace is reused by every call).  It never
 *     touches the old stream handle itself, so a caller may destroy that stream once
 *     its own work on it is done.
 *   - The placement pipeline's bounded links (fp_place_geometry FP_GEOM_BOUNDED) need the
 *     launch's segments co-resident.  Bounded launches of one process are serialised per
 *     device inside the library (each waits on its own stream for the previous one), so
 *     contexts on several host threads may plan at once; other launches only delay them.
 *     Only work of OTHER processes that holds the device's slots indefinitely can still
 *     end a bounded launch in FP_EDEVICE after the deadlock guard (60 s), never in a
 *     wrong plan.
 *   - Return 0 (FP_OK) or a negative FP_E* code.  There is no CPU fallback:
 *     fp_ctx_create fails with FP_EDEVICE when no MI355X (gfx950) is present.
 *   - One fp_ctx per host thread; contexts are not shared.
 *   - Integer semantics only; results are bit-exact with the CPU oracle
 *     (oracle/fp_oracle.c) by construction.  Semantics: SPEC.md.
 */
#ifndef FLEETPLACE_H
#define FLEETPLACE_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP_ABI_VERSION 1

#define FP_OK 0
#define FP_EINVAL (-1)     /* bad argument / inconsistent sizes                  */
#define FP_ENOMEM (-2)     /* device or host allocation failed                   */
#define FP_EDEVICE (-3)    /* no gfx950 device, or a HIP runtime error           */
#define FP_EOVERFLOW (-4)  /* a count exceeds uint32 / a packed-cost field       */
#define FP_ECORRUPT (-5)   /* input violates an invariant (e.g. CSR col >= V)    */

#define FP_NONE 0xFFFFFFFFu /* "no node" / "no level" (cycle)                    */

/* FP_REASON_SKEW: only from the *_policy_spread entries (SPEC.md 2.7): some node fits, none within max_skew
 * FP_REASON_QUOTA: only from the *_policy_quota entries (SPEC.md 2.10): the tenant's quota refuses the request */
enum fp_reason { FP_REASON_OK = 0, FP_REASON_NOFIT = 1, FP_REASON_CYCLE = 2, FP_REASON_SKEW = 3, FP_REASON_QUOTA = 4 };

typedef struct fp_ctx fp_ctx;

/* depends_on graph as a REVERSED CSR: row d lists the vertices that depend on d.
 * has_deps[v] = 1 iff v is known in flow.services and its depends_on is non-empty
 * (the engine.rs:71-80 predicate). */
typedef struct {
    uint32_t n_vertices, n_edges;
    const uint32_t *row_ptr;  /* [n_vertices + 1] */
    const uint32_t *col;      /* [n_edges]        */
    const uint8_t *has_deps;  /* [n_vertices]     */
} fp_graph;

/* Container requests, SoA: integer CPU millicores, memory MiB, required label
 * bits, conflict bits (host-port bits | anti-affinity group bits). */
typedef struct {
    uint32_t n;
    const uint32_t *cpu_m, *mem_mib, *req_labels, *conflict;
} fp_containers;

/* Node table, SoA, in node-index order (stage.servers order for KDL input,
 * ORDER BY slug for the controlplane registry, db.rs:741-750).  cpu_free,
 * mem_free and conflict_used are updated in place by placement. */
typedef struct {
    uint32_t n;
    uint32_t *cpu_free, *mem_free;
    const uint32_t *labels;
    uint32_t *conflict_used;
    const uint8_t *schedulable; /* 0 = cordon/drain (model.rs:435-442) */
} fp_nodes;

/* S independent what-if scenarios, each C containers on its own N nodes.
 * Every array is scenario-major: container arrays [S][C], node arrays [S][N].
 * scen_base + n_scen <= 65536 (the packed cost keeps a 16-bit scenario id), else
 * FP_EOVERFLOW. */
typedef struct {
    uint32_t n_scen, scen_base;   /* scen_base: global id of scenario 0 (cost field) */
    uint32_t n_containers, n_nodes;
    const uint32_t *cpu_m, *mem_mib, *req_labels, *conflict;
    const uint32_t *level;        /* [S][C] or NULL: FP_NONE => CYCLE, not placed   */
    uint32_t *cpu_free, *mem_free;
    const uint32_t *labels;
    uint32_t *conflict_used;
    const uint8_t *schedulable;
    uint32_t *assign;             /* [S][C] node index or FP_NONE                   */
    uint8_t *reason;              /* [S][C] enum fp_reason                          */
    uint64_t *cost;               /* [S] (n_rejected:24 | n_nodes_used:24 | id:16)  */
} fp_batch;

/* ---- context ------------------------------------------------------------ */
int fp_ctx_create(fp_ctx **out, int device);
void fp_ctx_destroy(fp_ctx *ctx);
/* Launch on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).
 * NULL selects the HIP null (default) stream; fp_ctx_reset_stream restores the
 * context's own non-blocking stream. */
int fp_ctx_set_stream(fp_ctx *ctx, void *hip_stream);
int fp_ctx_reset_stream(fp_ctx *ctx);
int fp_ctx_sync(fp_ctx *ctx);
const char *fp_strerror(int code);
int fp_abi_version(void);
/* Kernel timing (HIP events on the launch stream) for the roofline report.
 * kernel ids: see FP_K_* below. */
enum { FP_K_PLACE = 0, FP_K_SORT = 1, FP_K_FEAS = 2, FP_K_LEVEL = 3, FP_K_GEN = 4, FP_K_COUNT = 5 };
int fp_ctx_profile(fp_ctx *ctx, int enable);
int fp_ctx_kernel_stats(fp_ctx *ctx, int kernel_id, double *total_ms, uint64_t *launches);
/* The FFD kernel the last placement call on this context ran (waits for the stream): out[0] / out[1]
 * = the OR of every cpu / mem value of its batch (containers and schedulable nodes), out[2] = 1 for
 * the u32 records, 2 for the packed (cpu, mem) records (FP_OPT_PACKED), 3 for the packed records fed by
 * prepacked demand rows (FP_OPT_PREPACK), 4 for the u32 records after the repair pass turned prepacked rows
 * back into cpu / mem / position rows (a batch that does not pack as a whole), 0 if nothing ran.  All zero
 * also when a later call on the context has reused the workspace. */
int fp_ctx_place_path(fp_ctx *ctx, uint32_t *out3);

/* Per-context tuning / test options.  FP_OPT_AUTO (-1) = the production choice (the
 * default of every option).  Nothing is read from the environment: an option changes
 * only the context it is set on.  The pipeline geometry options are hints a shape may
 * not be able to serve (the planner then falls back to the nearest valid geometry);
 * fp_place_geometry reports what a call will run.  Results are bit-exact whatever the
 * options (only the work schedule changes); FP_OPT_SPIN_TICKS, and FP_OPT_LINK_BOUNDED = 1
 * on a batch whose segments are not all resident, can make a call fail with FP_EDEVICE
 * (never a wrong plan). */
#define FP_OPT_AUTO (-1)
enum fp_option {
    FP_OPT_PIPE_W = 0,        /* stages (waves) per segment, >= 1                         */
    FP_OPT_PIPE_SEG = 1,      /* 64-node groups per segment, 1..40                         */
    FP_OPT_PIPE_R = 2,        /* LDS ring depth between stages, 2..6                        */
    FP_OPT_PIPE_LAG = 3,      /* segment ticket lag (0 = segments side by side)            */
    FP_OPT_LINK_SLOTS = 4,    /* bounded global link ring slots, >= 8                       */
    FP_OPT_LINK_BOUNDED = 5,  /* 0 = links hold every container, 1 = bounded rings          */
    FP_OPT_PIPE_FLUSH = 6,    /* idle-flush mask: bit 0 LDS rings, bit 1 global links      */
    FP_OPT_SPIN_TICKS = 7,    /* deadlock guard in 100 MHz ticks (auto: 60 s)               */
    FP_OPT_KPACK = 8,         /* 0 = bucket search per stage instead of packed buckets      */
    FP_OPT_SCEN_SORT = 9,     /* 0 = radix-key FFD order instead of the per-scenario LDS sort */
    FP_OPT_SEGSORT = 10,      /* ignored (kept for ABI stability): the radix path is always   */
                              /* segmented for S > 1 and device-wide for S == 1             */
    FP_OPT_SYSTOLIC = 11,     /* systolic group fill for queues of >= value containers (0 = off) */
    FP_OPT_LEVELIZE_SYNC = 12,/* 1 = level-synchronous Kahn instead of the async levelizer */
    FP_OPT_SYSTOLIC_EXTRA = 13, /* systolic steps past the queue length before the serial finish */
    FP_OPT_SCREEN = 14,       /* 0 = no stage-2 early-NOFIT screen: every container enters    */
    FP_OPT_PAYLOAD_LDS = 15,  /* 0 = random-gather payload instead of the LDS-chunked one      */
    FP_OPT_SYSTOLIC_VALU = 16,/* systolic step loop: 0 exec-masked, 1 VALU-only, auto/2 DPP-folded */
    FP_OPT_LINK_PUBLISH = 17, /* full slots per head publish on unbounded global links (auto 32) */
    FP_OPT_LEVEL_SORT = 18,   /* levelizer start order: 0 = radix sort, auto = LSD counting sort   */
    FP_OPT_LEVEL_SMALL = 19,  /* 0 = no one-launch levelizer (<= 512 vertices) / legacy order (<= 1024);
                                 2 = fp_plan_stage without its one-wave path (<= 64 services)   */
    FP_OPT_PIPE_PRIO = 20,    /* FFD wave priority: 0 off, 1 raised in the group loop, 2 for a batch's work */
    FP_OPT_INDEG_BIN = 21,    /* 0 = levelizer in-degrees by global atomics instead of binned in LDS */
    FP_OPT_PACKED = 22,       /* 0 = FFD on u32 records only; auto = packed (cpu, mem) records when the
                                 batch's values fit them (decided on the device, fp_pipe_pk.h)  */
    FP_OPT_SORT_FUSED = 23,   /* 0 = the per-scenario sort and the LDS-chunked payload as two kernels; auto = one
                                 kernel (the payload is the sort's last phase), wherever both would run */
    FP_OPT_PREPACK = 24,      /* 0 = the fused sort always writes the cpu / mem / position rows; auto = one packed
                                 (cpu, mem) demand row per scenario whose values pack, wherever the packed
                                 4096-scenario kernel may run (decided on the device; plans are the same) */
    FP_OPT_COUNT = 25
};
int fp_ctx_set_option(fp_ctx *ctx, int option, int64_t value);
int fp_ctx_get_option(fp_ctx *ctx, int option, int64_t *value);

/* ---- host-pointer API (drop-in, synchronous) ---------------------------- */
/* A1 engine.rs:67-85: perm_out = stable partition (has_deps == 0 first). */
int fp_legacy_order(fp_ctx *ctx, const fp_graph *g, uint32_t *perm_out);
/* A2: level_out[v] (FP_NONE on/after a cycle), order_out = sort by (level, index).
 * n_cycle_out (nullable) receives the number of FP_NONE vertices. */
int fp_levelize(fp_ctx *ctx, const fp_graph *g, uint32_t *level_out, uint32_t *order_out,
                uint32_t *n_cycle_out);
/* A6: first-fit-decreasing; nodes mutated in place; level nullable. */
int fp_place(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level,
             uint32_t *assign_out, uint8_t *reason_out);
int fp_place_batch(fp_ctx *ctx, const fp_batch *b);
/* Scored placement (SPEC.md 2.6): containers in the FFD order of fp_place, same feasibility predicate
 * and CYCLE gating; among the feasible nodes the container goes to the one with the smallest key
 *   popcount(preferred_labels & ~labels[n]) << 58 | primary(n) << 26 | n
 * with primary(n) = 0 (FIRST_FIT), node_count[n] (SPREAD, `spread_across_pool`), cpu_free[n] - cpu_m
 * (PACK, `pack_into_dedicated`: best fit on CPU) or 0xFFFFFFFF - cpu_free[n] (FILL_LOWEST,
 * `fill_lowest`: most free CPU first); the strategies of the control plane's PlacementPolicy
 * (crates/fleetflow-controlplane/src/model.rs:56-95).  FIRST_FIT with preferred_labels = 0 is fp_place.
 * node_count ([N], or [S][N] for a batch; nullable) holds the containers already on each node and is
 * updated in place; NULL starts at zero and returns nothing.  The cost counts the nodes that received a
 * container in this call.  At most FP_POLICY_MAX_NODES nodes per scenario (FP_EOVERFLOW); a strategy
 * above FP_STRATEGY_FILL_LOWEST is FP_EINVAL. */
enum fp_strategy { FP_STRATEGY_FIRST_FIT = 0, FP_STRATEGY_SPREAD = 1, FP_STRATEGY_PACK = 2, FP_STRATEGY_FILL_LOWEST = 3 };
#define FP_POLICY_MAX_NODES 8192
int fp_place_policy(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level,
                    uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                    uint32_t *assign_out, uint8_t *reason_out);
/* strategy, preferred_labels: [S] per scenario (preferred_labels nullable = 0) */
int fp_place_batch_policy(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                          const uint32_t *preferred_labels, uint32_t *node_count);
/* Scored placement under a hard topology spread (SPEC.md 2.7), the PlacementPolicy's
 * SpreadConstraint{topology_key, max_skew} (model.rs:56-63; the counterpart of k8s PodTopologySpread with
 * whenUnsatisfiable = DoNotSchedule).  domain[n] < FP_SPREAD_MAX_DOMAINS is the topology domain of node n.
 * dom_count[d] = the sum of node_count[n] over the nodes of domain d (zero without node_count; u32, wraps);
 * a domain is eligible when one of its nodes is schedulable (fixed for the call, whatever the container).
 * A node is feasible when it is feasible for fp_place_policy and
 *   dom_count[domain[n]] - min(dom_count over the eligible domains) < max_skew
 * on the state the call's earlier placements left; among the feasible nodes fp_place_policy's key decides,
 * and a placement adds one to its domain's count.  A container some node fits but none within the skew is
 * FP_REASON_SKEW (counted as rejected in the cost); one no node fits stays FP_REASON_NOFIT.
 * max_skew = 0 is no constraint: that scenario is exactly fp_place_policy and its domain values are not read.
 * domain = NULL or max_skew = NULL (batch entries) is no constraint anywhere.  A domain value of
 * FP_SPREAD_MAX_DOMAINS or more in a scenario whose max_skew is not 0 is FP_EINVAL and nothing is written. */
#define FP_SPREAD_MAX_DOMAINS 64
int fp_place_policy_spread(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level,
                           uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                           const uint32_t *domain, uint32_t max_skew, uint32_t *assign_out, uint8_t *reason_out);
/* domain: [S][N]; max_skew: [S] */
int fp_place_batch_policy_spread(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                                 const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                                 const uint32_t *max_skew);
/* Scored placement under a fallback chain (SPEC.md 2.8), the PlacementPolicy's
 * FallbackPolicy{relax_order, max_hops} (model.rs:47-54): the required labels a container may give up, hop
 * by hop, when the pool that matches them has no feasible node.  relax_mask[h - 1] holds the label bits hop h
 * gives up (every key=value bit of one label key; any 32-bit masks are legal, they may overlap or be 0),
 * n_hops <= FP_FALLBACK_MAX_HOPS is the number of hops.  With cum[0] = 0, cum[h] = cum[h-1] | relax_mask[h-1]
 * and req_h = req_labels & ~cum[h], the hop of node n is the smallest h <= n_hops with
 * (labels[n] & req_h) == req_h.  A node is feasible when it is feasible for fp_place_policy_spread with
 * the label test replaced by "has a hop"; the container goes to the feasible node with the smallest
 * (hop, key), key being fp_place_policy's.  So a requirement is given up only when no node of any earlier
 * hop is feasible -- without capacity, in conflict, or outside max_skew.  hops_out (nullable) receives
 * the winner's hop, 0 for a rejected or CYCLE container.  FP_REASON_NOFIT: no node fits even under
 * req_{n_hops}; FP_REASON_SKEW: some node does, none within max_skew.  The cost is unchanged: a relaxed
 * placement counts as placed.  n_hops = 0 is no fallback: that scenario is exactly fp_place_policy_spread
 * and its relax_mask is not read.  relax_mask = NULL or n_hops = NULL (batch entries) is no fallback
 * anywhere.  domain = NULL or max_skew = NULL is still no spread constraint.  An n_hops above
 * FP_FALLBACK_MAX_HOPS is FP_EINVAL and nothing is written. */
#define FP_FALLBACK_MAX_HOPS 4
int fp_place_policy_fallback(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level,
                             uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                             const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                             uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out);
/* relax_mask: [S][FP_FALLBACK_MAX_HOPS]; n_hops: [S]; hops_out: [S][C] or NULL */
int fp_place_batch_policy_fallback(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                                   const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                                   const uint32_t *max_skew, const uint32_t *relax_mask, const uint32_t *n_hops,
                                   uint8_t *hops_out);
/* Scored placement under a resource quota (SPEC.md 2.10), the PlacementPolicy's ResourceQuota (model.rs:38-45;
 * the counterpart of a k8s ResourceQuota: admission before scheduling).  quota[d] caps what the tenant may hold
 * in dimension d -- FP_QUOTA_CPU in millicores, FP_QUOTA_MEM in MiB, FP_QUOTA_SERVICES in containers --
 * and FP_QUOTA_UNLIMITED is no cap there.  quota_used[d] (in/out, nullable: NULL starts at zero and returns
 * nothing, as node_count) is what the tenant holds already.  Containers are visited in the FFD order; a CYCLE
 * container is neither tested nor charged.  With r = (cpu_m, mem_mib, 1), dimension d blocks when
 *   quota[d] != FP_QUOTA_UNLIMITED && r[d] != 0 && !(used[d] <= quota[d] && r[d] <= quota[d] - used[d])
 * so a dimension the container asks nothing of is not tested, and a used above its cap blocks every
 * non-zero request.  A blocked container is FP_REASON_QUOTA (assign FP_NONE, hop 0, counted as rejected in the
 * cost) with the mask of the blocking dimensions (bit d) in quota_why_out; no node is searched and no state
 * changes.  Any other container is placed exactly as fp_place_policy_fallback places it, its quota_why is 0,
 * and when it is placed used[d] += r[d] in all three dimensions (u32, wraps; not under a finite cap).  NOFIT
 * and SKEW leave the usage as it was.  A quota of three FP_QUOTA_UNLIMITED is no quota: that scenario is
 * exactly fp_place_policy_fallback.  quota = NULL is no quota anywhere: the call is the _fallback entry, and
 * quota_used and quota_why_out are neither read nor written.  quota_why_out is nullable.  Every u32 is a legal
 * cap.  With no container to place quota_used stays as given.  ResourceQuota.max_stages is not a placement
 * input (it caps the tenant's stage records) and has no counterpart here. */
enum fp_quota_dim { FP_QUOTA_CPU = 0, FP_QUOTA_MEM = 1, FP_QUOTA_SERVICES = 2, FP_QUOTA_DIMS = 3 };
#define FP_QUOTA_UNLIMITED 0xFFFFFFFFu
/* quota, quota_used: [FP_QUOTA_DIMS]; quota_why_out: [C] */
int fp_place_policy_quota(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level,
                          uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                          const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                          uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out, const uint32_t *quota,
                          uint32_t *quota_used, uint8_t *quota_why_out);
/* quota, quota_used: [S][FP_QUOTA_DIMS]; quota_why_out: [S][C] */
int fp_place_batch_policy_quota(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                                const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                                const uint32_t *max_skew, const uint32_t *relax_mask, const uint32_t *n_hops,
                                uint8_t *hops_out, const uint32_t *quota, uint32_t *quota_used,
                                uint8_t *quota_why_out);
/* Stage 2: first feasible node (FP_NONE) and feasible-node count per container on
 * the given node state; bitmap_out (nullable, ceil(C/64) * N words) holds
 * bit (c, n) at word [(c/64) * N + n], bit c % 64. */
int fp_feasibility(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes,
                   uint32_t *first_out, uint32_t *count_out, uint64_t *bitmap_out);
/* Rejection diagnosis (SPEC.md 2.9): WHY a container has no node on the given node table -- the answer
 * "0/5 nodes available: 3 insufficient cpu, 2 didn't match the node selector".  Nothing is placed or mutated.
 * why(c, n) is the mask of the 2.3 predicates that fail for container c on node n, with
 * req' = req_labels[c] & ~ignore_labels (the label bits the caller gives up, e.g. a fallback chain's
 * cum[n_hops]); every bit is evaluated on every node, unschedulable nodes included, and why == 0 is exactly
 * "feasible by 2.3". */
enum fp_why { FP_WHY_CORDON = 1, FP_WHY_CPU = 2, FP_WHY_MEM = 4, FP_WHY_LABEL = 8, FP_WHY_CONFLICT = 16 };
/* One row of FP_EXPLAIN_WORDS u32 per explained container:
 *   FAIL[k]   nodes with bit k of why set (non-exclusive)      ONLY[k]  nodes with why == 1 << k (sole blocker)
 *   FEASIBLE  nodes with why == 0 (fp_feasibility's count when ignore_labels = 0)
 *   ALL       the AND of why over every node: what fails everywhere (0x1F when N = 0)
 *   MISSING   req' & ~(OR of labels over the schedulable nodes): required labels no schedulable node carries
 *   NEAR      the lowest node with exactly one bit of why set, else FP_NONE;  words 14, 15 are written as 0.
 * One histogram of FP_EXPLAIN_HIST_WORDS u32 per scenario, over its selected containers: words 0..4 count the
 * containers whose ALL has bit k (a container may count in several), MIXED those with FEASIBLE = 0 and ALL = 0,
 * FITS those with FEASIBLE > 0 (SKEW rejections, or a table that is not the final one), SELECTED all of them. */
enum { FP_EXPLAIN_FAIL = 0, FP_EXPLAIN_ONLY = 5, FP_EXPLAIN_FEASIBLE = 10, FP_EXPLAIN_ALL = 11,
       FP_EXPLAIN_MISSING = 12, FP_EXPLAIN_NEAR = 13, FP_EXPLAIN_WORDS = 16 };
enum { FP_EXPLAIN_HIST_MIXED = 5, FP_EXPLAIN_HIST_FITS = 6, FP_EXPLAIN_HIST_SELECTED = 7, FP_EXPLAIN_HIST_WORDS = 8 };
/* sel: n_sel container indices (< c->n, repeats allowed; one >= c->n is FP_EINVAL), or NULL = every container in
 * order (n_sel is then c->n whatever was passed).  rows_out: [n_sel][FP_EXPLAIN_WORDS].  After fp_place, or
 * fp_place_policy* without a spread constraint and with ignore_labels = cum[n_hops], every FP_REASON_NOFIT
 * container has FEASIBLE = 0 on the node table that call left (SPEC.md 2.3 monotonicity). */
int fp_explain(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *sel, uint32_t n_sel,
               uint32_t ignore_labels, uint32_t *rows_out);
/* Per-scenario histograms over b's containers and node state (e.g. the state fp_place_batch left).
 * reason_mask: bit r selects the containers with b->reason[s][c] == r; 0 = every container, b->reason is not
 * read.  ignore_labels: [S] or NULL = 0.  hist_out: [S][FP_EXPLAIN_HIST_WORDS].  Reads b's containers, node
 * state and reason; writes only hist_out.  n_scen <= 65535. */
int fp_explain_batch(fp_ctx *ctx, const fp_batch *b, uint32_t reason_mask, const uint32_t *ignore_labels,
                     uint32_t *hist_out);
/* Drain what-if sweep (SPEC.md 2.11): "can this server, or this whole zone, be taken out?", asked of every
 * candidate at once.  nodes is the LIVE table (every running container's request already deducted on its node),
 * assign[c] the node container c runs on (FP_NONE = not running), group[n] < n_cand the candidate node n belongs
 * to (FP_NONE = none): group[n] = n with n_cand = nodes->n drains each server alone, group = topology domain asks
 * about each zone's outage.  Every candidate k is computed independently from the same base state: its evictees
 * (the containers with group[assign[c]] == k) are visited in fp_place's order (cpu desc, mem desc, index asc)
 * and each goes to the feasible node with the smallest fp_place_policy key among the targets (schedulable and
 * group[n] != k), on the state the candidate's earlier moves left (cpu_free, mem_free, conflict_used and
 * node_count updated as fp_place_policy updates them).  Nothing is returned to the drained nodes and no input is
 * written.  assign_out[c] = the new node of a moved evictee, FP_NONE for a stranded one (reason_out
 * FP_REASON_NOFIT) and assign[c] for every other container (reason_out 0); the groups partition the nodes, so
 * the one array holds every candidate's plan.  summary_out holds one row of FP_DRAIN_WORDS u32 per candidate:
 *   EVICTED  its evictees        STRANDED  those left without a node      STRANDED_CPU, STRANDED_MEM  their sums
 *   TARGETS  the distinct nodes that received an evictee                  (u32, wrap)
 *   FIRST_STRANDED  the stranded container that comes first in the visiting order, else FP_NONE
 *   NODES    the nodes of the candidate;  word 7 is written as 0.
 * A candidate without evictees gets a row of zeros with FIRST_STRANDED = FP_NONE.  node_count is nullable
 * (zeros).  nodes->n or n_cand above FP_POLICY_MAX_NODES is FP_EOVERFLOW; a strategy above
 * FP_STRATEGY_FILL_LOWEST, assign_out == assign, a group[n] that is neither < n_cand nor FP_NONE and an
 * assign[c] that is neither < nodes->n nor FP_NONE are FP_EINVAL; on any error nothing is written.  The
 * policy's spread constraint and fallback chain are not applied to moves here: fp_drain_sweep_policy applies them. */
enum { FP_DRAIN_EVICTED = 0, FP_DRAIN_STRANDED = 1, FP_DRAIN_STRANDED_CPU = 2, FP_DRAIN_STRANDED_MEM = 3,
       FP_DRAIN_TARGETS = 4, FP_DRAIN_FIRST_STRANDED = 5, FP_DRAIN_NODES = 6, FP_DRAIN_WORDS = 8 };
int fp_drain_sweep(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                   const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                   const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out, uint32_t *summary_out);
/* The drain sweep under the policy (SPEC.md 2.15): fp_drain_sweep with every move held to the tenant's spread
 * constraint (domain[n] < FP_SPREAD_MAX_DOMAINS, max_skew; fp_place_policy_spread's meanings) and fallback chain
 * (relax_mask[n_hops], n_hops <= FP_FALLBACK_MAX_HOPS; fp_place_policy_fallback's).  There is no quota input: an
 * evictee is already charged to its tenant and a move releases and retakes the same request, so admission has
 * nothing to test.  Candidate k is exactly one fp_place_policy_fallback call over its evictees on the base table
 * with schedulable[n] &= group[n] != k and node_count[n] = 0 where group[n] == k: its domain counts leave its own
 * nodes out (what runs there is leaving; cordoned nodes outside it count), a domain is eligible when it has a
 * target, so a drained zone never holds the minimum down, and each evictee goes to the feasible target with the
 * smallest (hop, key) that passes the skew test on the candidate's running counts.  A stranded evictee is
 * FP_REASON_NOFIT when no target fits even under the last hop's requirement and FP_REASON_SKEW when one fits and
 * none passes; the summary row's STRANDED words and FIRST_STRANDED cover both.  hops_out (nullable) [c->n]: the
 * hop of a moved evictee, 0 for every other container.  policy_out (nullable) holds one row of
 * FP_DRAIN_POLICY_WORDS u32 per candidate:
 *   STRANDED_SKEW  evictees stranded on SKEW          RELAXED  evictees moved at a hop >= 1
 *   SKEW_BEFORE, SKEW_AFTER  max - min of the domain counts over the candidate's eligible domains, on its base
 *   counts and after its moves; both 0 when no domain is eligible or max_skew == 0.
 * A candidate without evictees gets a row of zeros.  domain == NULL or max_skew == 0: no constraint, domain is
 * not read; relax_mask == NULL or n_hops == 0: no chain; with neither the call is fp_drain_sweep bit for bit,
 * hops_out all 0 and the policy_out rows all 0.  Errors are fp_drain_sweep's, and n_hops above
 * FP_FALLBACK_MAX_HOPS or (with max_skew != 0) any domain[n] >= FP_SPREAD_MAX_DOMAINS, the candidate's nodes
 * included, are FP_EINVAL; on any error nothing is written. */
enum { FP_DRAIN_STRANDED_SKEW, FP_DRAIN_RELAXED, FP_DRAIN_SKEW_BEFORE, FP_DRAIN_SKEW_AFTER, /* words 0 to 3 */
       FP_DRAIN_POLICY_WORDS /* 4 */ };
int fp_drain_sweep_policy(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                          const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                          const uint32_t *node_count, const uint32_t *domain, uint32_t max_skew,
                          const uint32_t *relax_mask, uint32_t n_hops, uint32_t *assign_out, uint8_t *reason_out,
                          uint8_t *hops_out, uint32_t *summary_out, uint32_t *policy_out);
/* Scale-in sweep (SPEC.md 2.16): "which servers can I hand back, and what has to move so that I can?", asked of
 * every release order at once.  containers, nodes (the LIVE table), assign, strategy, preferred_labels and
 * node_count are fp_drain_sweep's.  Variant v is a release order try_order[v][0 .. n_try): node indices, FP_NONE
 * entries are skipped (ragged rows).  Every variant starts from the base state and is independent of the others.
 * Its entries are visited in order; an entry naming a node the variant already released is skipped; every other
 * entry is an ATTEMPT on its node n: the containers now on n are visited in fp_place's order and each goes to the
 * feasible node with the smallest fp_place_policy key among the targets (schedulable, not released, not n), on
 * the state the variant's committed attempts and this attempt's earlier moves left.  When every one finds a
 * target the attempt COMMITS (n is released; an attempt without containers commits with zero moves; a cordoned n
 * is attempted like any other).  At the first container no target takes (the BLOCKER) the attempt is UNDONE: the
 * state is exactly what it was before the attempt and n stays a target; a later entry naming n is a fresh attempt.
 *   assign_out  [n_var][c->n]      the variant's final assignment
 *   state_out   [n_var][nodes->n]  u8 per node: NEVER (not attempted), RELEASED, FAILED (its last attempt failed)
 *   blocker_out [n_var][nodes->n]  nullable: the blocker of a node in state FAILED, else FP_NONE
 *   summary_out [n_var][FP_SHRINK_WORDS]:
 *     RELEASED  nodes released      TRIED  attempts      FAILED  attempts undone (RELEASED + FAILED == TRIED)
 *     MOVES  committed moves, a container counts once per move      MOVED  containers with assign_out != assign
 *     MOVED_CPU, MOVED_MEM  the sums of the MOVED containers' requests (u32, wrap)
 *     FIRST_FAILED  the node of the first failed attempt, else FP_NONE
 * nodes->n above FP_POLICY_MAX_NODES, n_var above 65535 or c->n above 0x7FFF0000 (2^31 - 2^16: the positions the
 * kernel scans stay below 2^31) is FP_EOVERFLOW; a strategy above
 * FP_STRATEGY_FILL_LOWEST, assign_out == assign and an assign or try_order value that is neither < nodes->n nor
 * FP_NONE are FP_EINVAL;
 * on any error nothing is written.  n_var == 0 is FP_OK.  Zones as candidates, the policy's spread constraint,
 * fallback chain and quota, and the choice of the order are not part of this call. */
enum { FP_SHRINK_RELEASED = 0, FP_SHRINK_TRIED = 1, FP_SHRINK_FAILED = 2, FP_SHRINK_MOVES = 3, FP_SHRINK_MOVED = 4,
       FP_SHRINK_MOVED_CPU = 5, FP_SHRINK_MOVED_MEM = 6, FP_SHRINK_FIRST_FAILED = 7, FP_SHRINK_WORDS = 8 };
enum { FP_SHRINK_STATE_NEVER = 0, FP_SHRINK_STATE_RELEASED = 1, FP_SHRINK_STATE_FAILED = 2 };
int fp_shrink_sweep(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                    const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                    uint32_t preferred_labels, const uint32_t *node_count, uint32_t *assign_out, uint8_t *state_out,
                    uint32_t *blocker_out, uint32_t *summary_out);
/* The scale-in sweep under the policy (SPEC.md 2.17): fp_shrink_sweep with every move held to the tenant's spread
 * constraint (domain[n] < FP_SPREAD_MAX_DOMAINS, max_skew; fp_place_policy_spread's meanings) and fallback chain
 * (relax_mask[n_hops], n_hops <= FP_FALLBACK_MAX_HOPS; fp_place_policy_fallback's).  There is no quota input: a
 * move releases and retakes the same request.  An attempt on n is one fp_place_policy_fallback call over the
 * containers now on n, on the variant's current table with n and the released nodes unschedulable and their
 * node_count 0, cut at its first rejected container (the BLOCKER, whose reason is FP_REASON_NOFIT or
 * FP_REASON_SKEW as in fp_drain_sweep_policy).  A domain counts for the minimum while it holds a target of the
 * attempt.  BOUND RULE (under a spread constraint only): with skew(S) = max - min of the per-domain sums of the
 * running node_count over the unreleased nodes, taken over the domains that hold a schedulable unreleased node (0
 * without one), an attempt whose containers all found a target commits iff
 *     skew(after) <= max_skew || skew(after) <= skew(before)
 * where `before` is the state before the attempt (n counts) and `after` the state the commit would leave (n
 * released); otherwise it is undone like any failure, with blocker FP_NONE and reason FP_REASON_SKEW.
 *   hops_out           [n_var][c->n]      nullable: the hop of the container's last committed move, else 0
 *   blocker_reason_out [n_var][nodes->n]  nullable: FP_REASON_NOFIT / FP_REASON_SKEW for a node in state FAILED,
 *                                         else 0
 *   policy_out         [n_var][FP_SHRINK_POLICY_WORDS]  nullable:
 *     FAILED_SKEW  undone attempts whose reason is SKEW (blocker or bound rule)
 *     RELAXED      committed moves at a hop >= 1, counted like MOVES
 *     SKEW_BEFORE, SKEW_AFTER  skew of the base and of the final state; 0 without a constraint
 * domain == NULL or max_skew == 0: no constraint and domain is not read; relax_mask == NULL or n_hops == 0: no
 * chain; with neither the four results of fp_shrink_sweep are bit for bit that call's, hops_out and policy_out are
 * zeros and blocker_reason_out is FP_REASON_NOFIT on the FAILED nodes.  Errors: fp_shrink_sweep's, and FP_EINVAL
 * for n_hops > FP_FALLBACK_MAX_HOPS or (with max_skew != 0) any domain[n] >= FP_SPREAD_MAX_DOMAINS; on any error
 * nothing is written. */
enum { FP_SHRINK_FAILED_SKEW, FP_SHRINK_RELAXED, FP_SHRINK_SKEW_BEFORE, FP_SHRINK_SKEW_AFTER, /* words 0 to 3 */
       FP_SHRINK_POLICY_WORDS /* 4 */ };
int fp_shrink_sweep_policy(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                           const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                           uint32_t preferred_labels, const uint32_t *node_count, const uint32_t *domain,
                           uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops, uint32_t *assign_out,
                           uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out, uint8_t *hops_out,
                           uint8_t *blocker_reason_out, uint32_t *policy_out);
/* Rebalance sweep (SPEC.md 2.19; the SpreadConstraint of model.rs:56-63 on the live placements of model.rs:435-442):
 * "which seats do I have to give up so that the spread holds again, and where do they go?", asked of every victim
 * order at once.  containers, nodes (the LIVE table), assign, strategy and preferred_labels are fp_drain_sweep's;
 * domain / max_skew are fp_place_policy_spread's and relax_mask / n_hops fp_place_policy_fallback's.  node_count is
 * nullable and ABSENT MEANS DERIVED, not zero: node_count[n] = the number of c with assign[c] == n.  Variant v is a
 * victim order victim_order[v][0 .. n_try): container indices, FP_NONE entries are skipped (ragged rows), with the
 * move budget max_moves[v] (FP_NONE, or max_moves == NULL: unlimited).  Every variant starts from the base state and
 * is independent of the others.  With dom_count[d] the u32 sum of the running node_count over all nodes of domain d,
 * a domain eligible when it has a schedulable node, and min the least dom_count over the eligible domains, a domain
 * is HEAVY when it is eligible and dom_count[d] - min > max_skew.  The entries are visited in order; the variant
 * ends when its committed moves reach the budget (tested before every entry); an entry is skipped when it is
 * FP_NONE, its container does not run, or the domain of the node it runs on is not heavy.  Every other entry is an
 * ATTEMPT: the container is lifted off its node s (cpu_free, mem_free += its request, conflict_used &= ~conflict,
 * node_count -= 1) and placed exactly as the only container of an fp_place_policy_fallback call on that state.  If
 * a node takes it, that is a MOVE; otherwise the state is exactly what it was before the lift (the conflict word is
 * put back as it was) and the attempt is STUCK with that call's reason.  A repeated entry is a fresh attempt.
 *   assign_out  [n_var][c->n]  the variant's final assignment
 *   hops_out    [n_var][c->n]  nullable: the hop of the container's move, 0 if it never moved
 *   reason_out  [n_var][c->n]  nullable: FP_REASON_NOFIT / FP_REASON_SKEW if the container's last attempt was
 *                              rejected, else 0
 *   summary_out [n_var][FP_REBAL_WORDS]:
 *     MOVES  committed moves      STUCK  rejected attempts      STUCK_SKEW  those whose reason is SKEW
 *     RELAXED  moves at a hop >= 1      MOVED_CPU, MOVED_MEM  the sums of the moved containers' requests (u32, wrap)
 *     SKEW_BEFORE, SKEW_AFTER  max - min of dom_count over the eligible domains (0 without one), base and final state
 * domain == NULL or max_skew == 0: nothing is heavy, every assign_out row is assign, every other result is 0 and
 * domain is not read.  There is no quota input: a move releases and retakes the same request.  nodes->n above
 * FP_POLICY_MAX_NODES, n_var above 65535 or c->n above 0x7FFF0000 is FP_EOVERFLOW; a strategy above
 * FP_STRATEGY_FILL_LOWEST, n_hops above FP_FALLBACK_MAX_HOPS, assign_out == assign, a required pointer that is NULL,
 * an assign[c] that is neither < nodes->n nor FP_NONE, a victim_order entry that is neither < c->n nor FP_NONE and
 * (with max_skew != 0) a domain[n] >= FP_SPREAD_MAX_DOMAINS are FP_EINVAL; on any error nothing is written.
 * n_var == 0 is FP_OK.  Evicting for the quota, balancing utilisation without a spread constraint, the choice of
 * the victim order and the final node table are not part of this call. */
enum { FP_REBAL_MOVES = 0, FP_REBAL_STUCK = 1, FP_REBAL_STUCK_SKEW = 2, FP_REBAL_RELAXED = 3, FP_REBAL_MOVED_CPU = 4,
       FP_REBAL_MOVED_MEM = 5, FP_REBAL_SKEW_BEFORE = 6, FP_REBAL_SKEW_AFTER = 7, FP_REBAL_WORDS = 8 };
int fp_rebalance_sweep(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                       const uint32_t *victim_order, uint32_t n_var, uint32_t n_try, const uint32_t *max_moves,
                       uint32_t strategy, uint32_t preferred_labels, const uint32_t *node_count,
                       const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                       uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out);
/* Scale-out sweep (SPEC.md 2.12): "what do I have to add?", asked of every server template at once.  The pending
 * containers are those whose reason's bit is set in reason_mask (fp_explain_batch's convention; reason_mask == 0
 * selects every container and reason is not read and may be NULL).  Candidate k is a template: a new server has
 * cpu_free = t_cpu[k], mem_free = t_mem[k], labels = t_labels[k] (a plan string's size, provider.rs:15-30; the
 * labels and capacity a new server carries, model.rs:399-419), conflict_used = 0 and is schedulable.  Every
 * candidate is computed independently: fp_place of the pending containers on t_max[k] such servers (t_max NULL =
 * max_new for every candidate; max_new <= FP_GROW_MAX_NEW is the most any candidate may open).  The servers are
 * identical, so the used ones are [0, OPENED).  summary_out holds one row of FP_GROW_WORDS u32 per candidate:
 *   PENDING  the number pending (the same in every row)     PLACED  those that got a new server
 *   OPENED   new servers used                                UNPLACEABLE  pending that no such server can take
 *   CAPPED   the rest: room ran out within t_max[k]          (cpu_m > t_cpu || mem_mib > t_mem || labels missing)
 *   LEFT_CPU, LEFT_MEM  what is free on the OPENED servers at the end (u32, wrap)
 *   FIRST_UNPLACED  the first container in visiting order that is UNPLACEABLE or CAPPED, else FP_NONE
 * PENDING == PLACED + UNPLACEABLE + CAPPED.  assign_out (nullable) is [n_cand][c->n]: the ordinal in [0, OPENED)
 * of the new server a placed pending container got, FP_NONE for every other container.  No input is written.
 * n_cand > 65535 or max_new > FP_GROW_MAX_NEW is FP_EOVERFLOW; reason == NULL with reason_mask != 0 and a
 * t_max[k] > max_new are FP_EINVAL; on any error nothing is written.  Only first fit; preferred labels, the
 * spread constraint, the fallback chain and the quota are not applied: fp_grow_sweep_policy applies them. */
enum { FP_GROW_PENDING = 0, FP_GROW_PLACED = 1, FP_GROW_OPENED = 2, FP_GROW_UNPLACEABLE = 3, FP_GROW_CAPPED = 4,
       FP_GROW_LEFT_CPU = 5, FP_GROW_LEFT_MEM = 6, FP_GROW_FIRST_UNPLACED = 7, FP_GROW_WORDS = 8 };
#define FP_GROW_MAX_NEW 8192u
int fp_grow_sweep(fp_ctx *ctx, const fp_containers *c, const uint8_t *reason, uint32_t reason_mask,
                  uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                  const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out);
/* The scale-out sweep under the policy (SPEC.md 2.18): "what do I have to add, and WHERE?", for a tenant whose
 * PlacementPolicy carries a strategy, preferred labels, a spread constraint, a fallback chain and a quota.
 * c, reason, reason_mask, the templates, t_max and max_new are fp_grow_sweep's.  nodes is the LIVE table (read
 * only; nodes->n may be 0), node_count its counts (nullable: zeros), domain[n] the live nodes' topology domains and
 * t_domain[k] the domain a new server of template k stands in (both < FP_SPREAD_MAX_DOMAINS; a new domain is an id
 * no live node has).  relax_mask[n_hops] is fp_place_policy_fallback's; quota[FP_QUOTA_DIMS] and
 * quota_used[FP_QUOTA_DIMS] are fp_place_policy_quota's, both nullable, quota_used READ ONLY here: a pending
 * container is not charged to its tenant yet, so admission has something to test.
 * Candidate k is computed independently and writes no input.  It is exactly one fp_place_policy_quota call over the
 * pending containers on the live table followed by M = t_max[k] template nodes (cpu_free = t_cpu[k], mem_free =
 * t_mem[k], labels = t_labels[k], conflict_used = 0, schedulable, node_count = 0, domain = t_domain[k]) under the
 * call's strategy, preferred labels, constraint, chain, quota and usage.  So the template's domain is eligible as
 * soon as M >= 1, a new domain starts at count 0, and a pending container may land on a LIVE node (filling a
 * starved domain raises the minimum and reopens the domains the skew test had closed).
 * summary_out is fp_grow_sweep's row, read by the reason that call gives:
 *   PLACED  reason OK, on a live or a new node          OPENED  new nodes that received a container: [N, N + OPENED)
 *   UNPLACEABLE  reason NOFIT and cpu_m > t_cpu || mem_mib > t_mem || (t_labels & req') != req', with
 *                req' = req_labels & ~cum[n_hops]        CAPPED  reason NOFIT otherwise
 *   LEFT_CPU, LEFT_MEM  summed over the OPENED new servers     FIRST_UNPLACED  the first pending with reason != 0
 * policy_out (nullable) holds one row of FP_GROW_POLICY_WORDS u32 per candidate:
 *   ON_LIVE  placed on a node < nodes->n     RELAXED  placed at a hop >= 1
 *   STUCK_SKEW  reason SKEW                   STUCK_QUOTA  reason QUOTA
 *   SKEW_BEFORE, SKEW_AFTER  max - min of the domain counts over the eligible domains of the combined table,
 *   before and after; 0 without a constraint or without an eligible domain.  Words 6 and 7 are written as 0.
 * PENDING == PLACED + UNPLACEABLE + CAPPED + STUCK_SKEW + STUCK_QUOTA.  The nullable [n_cand][c->n] results:
 * assign_out = the node in the combined table (nodes->n + j is the j-th new server), FP_NONE for every container
 * that is not pending or not placed; hops_out = the hop, else 0; reason_out = the reason, 0 for every container
 * that is not pending or placed.  With nothing pending every row is zeros with FIRST_UNPLACED = FP_NONE.
 * t_domain == NULL or max_skew == 0: no constraint, neither domain array is read; relax_mask == NULL or n_hops ==
 * 0: no chain; quota == NULL: no quota, quota_used is not read.  With nodes->n == 0, first fit, no preferred labels
 * and none of the three, summary_out and assign_out are fp_grow_sweep's bit for bit.
 * Errors: fp_grow_sweep's, with nodes->n + max_new > FP_POLICY_MAX_NODES as FP_EOVERFLOW; a strategy above
 * FP_STRATEGY_FILL_LOWEST, n_hops > FP_FALLBACK_MAX_HOPS, domain == NULL with a constraint and nodes->n != 0, and
 * (with max_skew != 0) any domain[n] or t_domain[k] >= FP_SPREAD_MAX_DOMAINS, whatever t_max[k] is, are FP_EINVAL;
 * on any error nothing is written. */
enum { FP_GROW_ON_LIVE, FP_GROW_RELAXED, FP_GROW_STUCK_SKEW, FP_GROW_STUCK_QUOTA, FP_GROW_SKEW_BEFORE,
       FP_GROW_SKEW_AFTER, /* words 0 to 5 */ FP_GROW_POLICY_WORD6, FP_GROW_POLICY_WORD7, /* written as 0 */
       FP_GROW_POLICY_WORDS /* 8 */ };
int fp_grow_sweep_policy(fp_ctx *ctx, const fp_containers *c, const uint8_t *reason, uint32_t reason_mask,
                         const fp_nodes *nodes, const uint32_t *node_count, uint32_t n_cand, const uint32_t *t_cpu,
                         const uint32_t *t_mem, const uint32_t *t_labels, const uint32_t *t_max, uint32_t max_new,
                         uint32_t strategy, uint32_t preferred_labels, const uint32_t *domain,
                         const uint32_t *t_domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                         const uint32_t *quota, const uint32_t *quota_used, uint32_t *summary_out,
                         uint32_t *policy_out, uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out);
/* Re-planning a running stage (SPEC.md 2.13): fp_place_policy that knows where each container runs now.  nodes is
 * the BASE table (everything deducted except these containers' own requests) and is updated in place; prev[c] is
 * the node container c runs on, < nodes->n, or FP_NONE.  Pass 1 (seats) visits the containers in fp_place's order
 * (cpu desc, mem desc, index asc), skipping CYCLE containers and those with prev == FP_NONE: a container keeps
 * n = prev[c] iff cpu_free[n] >= cpu_m, mem_free[n] >= mem_mib, (labels[n] & req) == req and
 * (conflict_used[n] & conflict) == 0 on the state the earlier seats left -- fp_place's predicate without
 * `schedulable`: a cordoned node keeps what runs on it.  A kept container updates its node as fp_place_policy does
 * (node_count += 1 included); assign = prev, reason OK, change KEPT.  Pass 2 visits, in the same order, every
 * container that is neither CYCLE nor kept and places it exactly as fp_place_policy does (schedulable included) on
 * the state pass 1 left: reason OK or NOFIT.  A CYCLE container is assign FP_NONE, reason CYCLE, whatever its prev.
 * The cost counts NOFIT + CYCLE as rejected and the nodes that received a container in either pass.
 * change_out (nullable) holds one enum fp_change per container; summary_out (nullable) one row of FP_REPLAN_WORDS
 * u32 per scenario: words 0..4 the number of containers with each change value, MOVED_CPU / MOVED_MEM the sums of
 * the MOVED containers' requests (the migration volume; u32, wrap), word 7 written as 0.
 * prev all FP_NONE is exactly fp_place_policy; prev = the assign of an fp_place_policy call on the same inputs
 * returns that call's outputs with every placed container KEPT.  nodes->n above FP_POLICY_MAX_NODES is
 * FP_EOVERFLOW; a strategy above FP_STRATEGY_FILL_LOWEST, prev == assign_out (the same buffer read and written) and
 * a prev[c] that is neither < nodes->n nor FP_NONE are FP_EINVAL; on any error nothing is written.  The policy's
 * spread constraint, fallback chain and quota are not applied, and no capacity is handed back from a live table:
 * the caller passes the base table. */
enum fp_change { FP_CHANGE_KEPT = 0, FP_CHANGE_NEW = 1, FP_CHANGE_MOVED = 2, FP_CHANGE_LOST = 3, FP_CHANGE_ABSENT = 4 };
enum { FP_REPLAN_KEPT = 0, FP_REPLAN_NEW = 1, FP_REPLAN_MOVED = 2, FP_REPLAN_LOST = 3, FP_REPLAN_ABSENT = 4,
       FP_REPLAN_MOVED_CPU = 5, FP_REPLAN_MOVED_MEM = 6, FP_REPLAN_WORDS = 8 };
int fp_replan(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level, const uint32_t *prev,
              uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count, uint32_t *assign_out,
              uint8_t *reason_out, uint8_t *change_out, uint32_t *summary_out);
/* prev: [S][C]; strategy, preferred_labels: [S] (preferred_labels nullable = 0); node_count: [S][N] or NULL;
 * change_out: [S][C] or NULL; summary_out: [S][FP_REPLAN_WORDS] or NULL.  prev == b->assign is FP_EINVAL. */
int fp_replan_batch(fp_ctx *ctx, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                    const uint32_t *preferred_labels, uint32_t *node_count, uint8_t *change_out,
                    uint32_t *summary_out);
/* Re-planning under the tenant's policy (SPEC.md 2.14): fp_replan with the spread constraint, the fallback chain and
 * the resource quota of fp_place_policy_quota, whose arguments these are and in whose order they stand; every one of
 * them is nullable with the meaning it has there (domain NULL or max_skew 0: no constraint; relax_mask NULL or n_hops
 * 0: no chain; quota NULL: no quota, and quota_used and quota_why_out are not touched).
 * Pass 1 (seats) is fp_replan's, with the labels tested under the whole chain, req & ~cum[n_hops]; there is NO skew
 * test and NO quota test: the guarantees gate the admission of new placements, they count what runs and never evict
 * it (k8s PodTopologySpread and ResourceQuota).  A kept container's hop is the first hop at which prev's labels
 * match, its quota_why is 0, and it is charged: used[d] += r[d] in all three dimensions (u32, wraps).
 * Pass 2 places every container that is neither CYCLE nor kept exactly as fp_place_policy_quota would, on the state
 * pass 1 left: the node table, the counts -- seats count in their domains, on cordoned nodes too -- and the usage
 * with the seats' charges; a usage the seats put above a cap blocks every non-zero request in that dimension.
 * Reasons OK, NOFIT, SKEW, QUOTA and CYCLE; change_out and summary_out as fp_replan's, FP_CHANGE_LOST covering every
 * rejection of a container that had a prev.  So no new or moved placement breaks the skew bound relative to the
 * current counts or is admitted past a cap, while the seats alone may leave max - min > max_skew or a usage above
 * a cap.  Without any guarantee the call is fp_replan; with prev all FP_NONE it is fp_place_policy_quota.
 * The errors are fp_replan's and fp_place_policy_fallback's (a domain id >= FP_SPREAD_MAX_DOMAINS in a scenario
 * with max_skew != 0, n_hops > FP_FALLBACK_MAX_HOPS: FP_EINVAL); on any error nothing is written, quota_used
 * included. */
int fp_replan_policy(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level, const uint32_t *prev,
                     uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count, const uint32_t *domain,
                     uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops, uint32_t *assign_out,
                     uint8_t *reason_out, uint8_t *hops_out, const uint32_t *quota, uint32_t *quota_used,
                     uint8_t *quota_why_out, uint8_t *change_out, uint32_t *summary_out);
/* The batch form: the arrays of fp_replan_batch and of fp_place_batch_policy_quota, per scenario. */
int fp_replan_batch_policy(fp_ctx *ctx, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                           const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                           const uint32_t *max_skew, const uint32_t *relax_mask, const uint32_t *n_hops,
                           uint8_t *hops_out, const uint32_t *quota, uint32_t *quota_used, uint8_t *quota_why_out,
                           uint8_t *change_out, uint32_t *summary_out);
/* One stage's whole plan, the `fleet up --dry-run` path (crates/fleetflow/src/commands/up.rs:57-136):
 *   perm_out                 A1 legacy start order (engine.rs:64-85, as fp_legacy_order)
 *   level_out, order_out, n_cycle_out   A2 levels and start order (as fp_levelize)
 * and, when nodes is not NULL (a stage with servers; c->n == n_vertices, container v = vertex v):
 *   first_out, count_out     stage 2 on the pristine table (as fp_feasibility; nullable)
 *   assign_out, reason_out   A6 first-fit-decreasing gated by the levels' CYCLE (as fp_place);
 *                            nodes updated in place.
 * A stage of <= 512 services, <= 8192 edges and <= 4096 servers is ONE kernel reading its inputs
 * from and writing its results to mapped pinned host memory (one launch and one synchronisation,
 * no copy calls: BASELINE config 1); larger stages run the general kernels.  FP_OPT_LEVEL_SMALL = 0
 * forces the general path.  Synchronous; on error nothing is written. */
int fp_plan_stage(fp_ctx *ctx, const fp_graph *g, const fp_containers *c, fp_nodes *nodes,
                  uint32_t *perm_out, uint32_t *level_out, uint32_t *order_out, uint32_t *n_cycle_out,
                  uint32_t *first_out, uint32_t *count_out, uint32_t *assign_out, uint8_t *reason_out);

/* ---- device-pointer API (async on the ctx stream) ----------------------- */
int fp_dev_legacy_order(fp_ctx *ctx, const fp_graph *g, uint32_t *perm_out);
int fp_dev_levelize(fp_ctx *ctx, const fp_graph *g, uint32_t *level_out, uint32_t *order_out,
                    uint32_t *n_cycle_out_dev);
int fp_dev_place_batch(fp_ctx *ctx, const fp_batch *b);
/* Device workspace (bytes) fp_place_batch / fp_dev_place_batch take on this ctx for
 * n_scen scenarios of n_containers x n_nodes (0 when there is nothing to place); the ctx
 * grows its workspace to it on the first such call and keeps it.  Depends on the device
 * (the pipeline's link sizing follows its occupancy). */
int fp_place_ws_bytes(fp_ctx *ctx, uint32_t n_scen, uint32_t n_containers, uint32_t n_nodes,
                      uint64_t *bytes_out);
/* The placement pipeline a batch of n_scen x n_containers x n_nodes runs on this ctx and
 * device (options included): out[FP_GEOM_*]. */
enum { FP_GEOM_GROUPS = 0, FP_GEOM_STAGES = 1, FP_GEOM_SEGMENTS = 2, FP_GEOM_RING = 3, FP_GEOM_LAG = 4,
       FP_GEOM_LINK_SLOTS = 5, FP_GEOM_BOUNDED = 6, FP_GEOM_RESIDENT = 7, FP_GEOM_SYSTOLIC = 8,
       FP_GEOM_COUNT = 9 };
int fp_place_geometry(fp_ctx *ctx, uint32_t n_scen, uint32_t n_containers, uint32_t n_nodes, uint32_t *out);
int fp_dev_feasibility(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes,
                       uint32_t *first_out, uint32_t *count_out, uint64_t *bitmap_out);
/* Stage 2 batched over what-if scenarios: for each scenario s and container c of b
 * (b's containers and node state; nothing is placed or mutated), first_out[s*C + c] = the
 * lowest feasible node (FP_NONE if none) and count_out[s*C + c] = the number of feasible
 * nodes.  n_scen <= 65535. */
int fp_dev_feasibility_batch(fp_ctx *ctx, const fp_batch *b, uint32_t *first_out, uint32_t *count_out);
/* As fp_explain on device pointers; rows_out is 64-byte aligned (else FP_EINVAL).  A sel index >= c->n is found
 * on the device before any row is written: no row is written and fp_ctx_sync() reports FP_ECORRUPT. */
int fp_dev_explain(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *sel, uint32_t n_sel,
                   uint32_t ignore_labels, uint32_t *rows_out);
/* As fp_explain_batch on device pointers.  The selection is compacted on the device; the call takes at most
 * 8 bytes per container of the batch plus 4 per scenario from the context's workspace. */
int fp_dev_explain_batch(fp_ctx *ctx, const fp_batch *b, uint32_t reason_mask, const uint32_t *ignore_labels,
                         uint32_t *hist_out);
/* As fp_place_batch_policy on device pointers (strategy, preferred_labels and node_count included).
 * A strategy value that is no fp_strategy is found on the device: nothing is written and
 * fp_ctx_sync() reports FP_EINVAL. */
int fp_dev_place_batch_policy(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                              const uint32_t *preferred_labels, uint32_t *node_count);
/* As fp_place_batch_policy_spread on device pointers.  A domain value that is out of range is found on
 * the device with the strategy check: nothing is written and fp_ctx_sync() reports FP_EINVAL. */
int fp_dev_place_batch_policy_spread(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                                     const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                                     const uint32_t *max_skew);
/* As fp_place_batch_policy_fallback on device pointers.  An n_hops above FP_FALLBACK_MAX_HOPS is found on
 * the device with the strategy check: nothing is written and fp_ctx_sync() reports FP_EINVAL. */
int fp_dev_place_batch_policy_fallback(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                                       const uint32_t *preferred_labels, uint32_t *node_count,
                                       const uint32_t *domain, const uint32_t *max_skew, const uint32_t *relax_mask,
                                       const uint32_t *n_hops, uint8_t *hops_out);
/* As fp_place_batch_policy_quota on device pointers.  The errors are those of fp_dev_place_batch_policy_fallback
 * (a quota has no illegal value): nothing is written, quota_used and quota_why_out included. */
int fp_dev_place_batch_policy_quota(fp_ctx *ctx, const fp_batch *b, const uint32_t *strategy,
                                    const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                                    const uint32_t *max_skew, const uint32_t *relax_mask, const uint32_t *n_hops,
                                    uint8_t *hops_out, const uint32_t *quota, uint32_t *quota_used,
                                    uint8_t *quota_why_out);
/* As fp_drain_sweep on device pointers (summary_out included).  A group or assign value out of range is found
 * on the device before any store: nothing is written and fp_ctx_sync() reports FP_EINVAL.  The call takes 24
 * bytes per container plus the sorts' scratch from the context's workspace. */
int fp_dev_drain_sweep(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                       const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                       const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out,
                       uint32_t *summary_out);
/* As fp_drain_sweep_policy on device pointers, with ONE exception to "fp_dev_* take device pointers":
 * relax_mask is a HOST array of n_hops words, read during the call like the scalars beside it (the cumulative
 * masks go to the kernel by value); n_hops above FP_FALLBACK_MAX_HOPS is returned directly.  A group, assign or
 * domain value out of range is found on the device before any store: nothing is written, hops_out and policy_out
 * included, and fp_ctx_sync() reports FP_EINVAL.  Workspace as fp_dev_drain_sweep. */
int fp_dev_drain_sweep_policy(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                              const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                              const uint32_t *node_count, const uint32_t *domain, uint32_t max_skew,
                              const uint32_t *relax_mask, uint32_t n_hops, uint32_t *assign_out,
                              uint8_t *reason_out, uint8_t *hops_out, uint32_t *summary_out, uint32_t *policy_out);
/* As fp_shrink_sweep on device pointers (every output included).  An assign or try_order value out of range is
 * found on the device before any store: nothing is written and fp_ctx_sync() reports FP_EINVAL.  The call takes
 * the FFD order's 24 bytes per container plus the sort's scratch and 12 bytes per container and variant (one of
 * the three words rounded up to a multiple of 16384 containers, of 1024 with at most 64 nodes) from the context's
 * workspace. */
int fp_dev_shrink_sweep(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                        const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                        uint32_t preferred_labels, const uint32_t *node_count, uint32_t *assign_out,
                        uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out);
/* As fp_shrink_sweep_policy on device pointers (every output included; relax_mask stays a HOST array of n_hops
 * words: the masks go to the kernel by value); n_hops above FP_FALLBACK_MAX_HOPS is returned directly.  An assign,
 * try_order or domain value out of range is found on the device before any store: nothing is written and
 * fp_ctx_sync() reports FP_EINVAL.  The workspace is fp_dev_shrink_sweep's. */
int fp_dev_shrink_sweep_policy(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                               const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                               uint32_t preferred_labels, const uint32_t *node_count, const uint32_t *domain,
                               uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops, uint32_t *assign_out,
                               uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out, uint8_t *hops_out,
                               uint8_t *blocker_reason_out, uint32_t *policy_out);
/* As fp_rebalance_sweep on device pointers (every output included; relax_mask stays a HOST array of n_hops words:
 * the masks go to the kernel by value; model.rs:56-63 and :435-442 as there).  A strategy above
 * FP_STRATEGY_FILL_LOWEST and n_hops above FP_FALLBACK_MAX_HOPS are returned directly.  An assign, victim_order or
 * domain value out of range is found on the device before any store: nothing is written and fp_ctx_sync() reports
 * FP_EINVAL.  The call takes 256 bytes, and 4 bytes per node where node_count is NULL, from the context's
 * workspace; the variants' running rows are the assign_out rows. */
int fp_dev_rebalance_sweep(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes, const uint32_t *assign,
                           const uint32_t *victim_order, uint32_t n_var, uint32_t n_try, const uint32_t *max_moves,
                           uint32_t strategy, uint32_t preferred_labels, const uint32_t *node_count,
                           const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                           uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out);
/* As fp_grow_sweep on device pointers (max_new stays a host value: the kernel's geometry follows it, nothing is
 * read back).  A t_max[k] > max_new is found on the device before any store: nothing is written and fp_ctx_sync()
 * reports FP_EINVAL.  The call takes 28 bytes per container plus the sort's scratch from the context's workspace. */
int fp_dev_grow_sweep(fp_ctx *ctx, const fp_containers *c, const uint8_t *reason, uint32_t reason_mask,
                      uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                      const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out);
/* As fp_grow_sweep_policy on device pointers, with the exceptions of fp_dev_drain_sweep_policy and one more:
 * relax_mask (n_hops words), quota and quota_used (FP_QUOTA_DIMS words each) are HOST arrays, read during the call
 * like the scalars beside them; max_new stays a host value and the geometry follows nodes->n + max_new.  A strategy
 * above FP_STRATEGY_FILL_LOWEST and n_hops above FP_FALLBACK_MAX_HOPS are returned directly.  A t_max[k] > max_new
 * or a domain / t_domain value out of range is found on the device before any store: nothing is written and
 * fp_ctx_sync() reports FP_EINVAL.  Workspace as fp_dev_grow_sweep. */
int fp_dev_grow_sweep_policy(fp_ctx *ctx, const fp_containers *c, const uint8_t *reason, uint32_t reason_mask,
                             const fp_nodes *nodes, const uint32_t *node_count, uint32_t n_cand,
                             const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                             const uint32_t *t_max, uint32_t max_new, uint32_t strategy, uint32_t preferred_labels,
                             const uint32_t *domain, const uint32_t *t_domain, uint32_t max_skew,
                             const uint32_t *relax_mask, uint32_t n_hops, const uint32_t *quota,
                             const uint32_t *quota_used, uint32_t *summary_out, uint32_t *policy_out,
                             uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out);
/* As fp_replan_batch on device pointers (change_out and summary_out included).  A strategy that is no fp_strategy
 * value and a prev value out of range are found on the device before any store: nothing is written and
 * fp_ctx_sync() reports FP_EINVAL.  The call takes the FFD order's 24 bytes per container plus the sort's scratch
 * and one byte per container from the context's workspace. */
int fp_dev_replan_batch(fp_ctx *ctx, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                        const uint32_t *preferred_labels, uint32_t *node_count, uint8_t *change_out,
                        uint32_t *summary_out);
/* As fp_replan_batch_policy on device pointers.  A strategy, prev, domain or n_hops value out of range is found on
 * the device before any store: nothing is written, quota_used included, and fp_ctx_sync() reports FP_EINVAL.  The
 * call takes the FFD order's 24 bytes per container plus the sort's scratch from the context's workspace (which
 * container was kept is marked in a buffer of the order's); without any guarantee it is fp_dev_replan_batch,
 * with 256 bytes more when hops_out is given. */
int fp_dev_replan_batch_policy(fp_ctx *ctx, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                               const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                               const uint32_t *max_skew, const uint32_t *relax_mask, const uint32_t *n_hops,
                               uint8_t *hops_out, const uint32_t *quota, uint32_t *quota_used,
                               uint8_t *quota_why_out, uint8_t *change_out, uint32_t *summary_out);
/* Best plan over a cost vector (device): writes the argmin index to *best_dev. */
int fp_dev_argmin_cost(fp_ctx *ctx, const uint64_t *cost, uint32_t n, uint32_t *best_dev);

/* ---- synthetic inputs (SPEC.md section 3), device-side ------------------- */
/* flags: bit0 host ports, bit1 anti-affinity groups, bit2 required labels. */
int fp_dev_gen_batch(fp_ctx *ctx, uint64_t seed, const fp_batch *b, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif
