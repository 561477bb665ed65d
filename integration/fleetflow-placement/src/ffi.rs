//! Raw bindings of include/fleetplace.h (ABI version 1).  Every `#[repr(C)]` struct here
//! mirrors the C struct field for field; tests/test_rust_binding.py checks that they
//! stay in step with the header.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const FP_ABI_VERSION: c_int = 1;
pub const FP_OK: c_int = 0;
pub const FP_EINVAL: c_int = -1;
pub const FP_ENOMEM: c_int = -2;
pub const FP_EDEVICE: c_int = -3;
pub const FP_EOVERFLOW: c_int = -4;
pub const FP_ECORRUPT: c_int = -5;
pub const FP_NONE: u32 = 0xFFFF_FFFF;
pub const FP_REASON_OK: u8 = 0;
pub const FP_REASON_NOFIT: u8 = 1;
pub const FP_REASON_CYCLE: u8 = 2;
pub const FP_REASON_SKEW: u8 = 3;
pub const FP_REASON_QUOTA: u8 = 4;
pub const FP_STRATEGY_FIRST_FIT: u32 = 0;
pub const FP_STRATEGY_SPREAD: u32 = 1;
pub const FP_STRATEGY_PACK: u32 = 2;
pub const FP_STRATEGY_FILL_LOWEST: u32 = 3;
pub const FP_POLICY_MAX_NODES: u32 = 8192;
pub const FP_SPREAD_MAX_DOMAINS: u32 = 64;
pub const FP_FALLBACK_MAX_HOPS: u32 = 4;
// resource quota (SPEC.md 2.10): enum fp_quota_dim (the index in a quota row and the bit in quota_why)
pub const FP_QUOTA_CPU: usize = 0;
pub const FP_QUOTA_MEM: usize = 1;
pub const FP_QUOTA_SERVICES: usize = 2;
pub const FP_QUOTA_DIMS: usize = 3;
pub const FP_QUOTA_UNLIMITED: u32 = 0xFFFF_FFFF;
// rejection diagnosis (SPEC.md 2.9): enum fp_why, the word indices of a row and of a histogram
pub const FP_WHY_CORDON: u32 = 1;
pub const FP_WHY_CPU: u32 = 2;
pub const FP_WHY_MEM: u32 = 4;
pub const FP_WHY_LABEL: u32 = 8;
pub const FP_WHY_CONFLICT: u32 = 16;
pub const FP_EXPLAIN_FAIL: usize = 0;
pub const FP_EXPLAIN_ONLY: usize = 5;
pub const FP_EXPLAIN_FEASIBLE: usize = 10;
pub const FP_EXPLAIN_ALL: usize = 11;
pub const FP_EXPLAIN_MISSING: usize = 12;
pub const FP_EXPLAIN_NEAR: usize = 13;
pub const FP_EXPLAIN_WORDS: usize = 16;
pub const FP_EXPLAIN_HIST_MIXED: usize = 5;
pub const FP_EXPLAIN_HIST_FITS: usize = 6;
pub const FP_EXPLAIN_HIST_SELECTED: usize = 7;
pub const FP_EXPLAIN_HIST_WORDS: usize = 8;
// drain what-if sweep (SPEC.md 2.11): the word indices of a candidate's summary row
pub const FP_DRAIN_EVICTED: usize = 0;
pub const FP_DRAIN_STRANDED: usize = 1;
pub const FP_DRAIN_STRANDED_CPU: usize = 2;
pub const FP_DRAIN_STRANDED_MEM: usize = 3;
pub const FP_DRAIN_TARGETS: usize = 4;
pub const FP_DRAIN_FIRST_STRANDED: usize = 5;
pub const FP_DRAIN_NODES: usize = 6;
pub const FP_DRAIN_WORDS: usize = 8;
// scale-in sweep (SPEC.md 2.16): the word indices of a variant's summary row and the values of a node's state
pub const FP_SHRINK_RELEASED: usize = 0;
pub const FP_SHRINK_TRIED: usize = 1;
pub const FP_SHRINK_FAILED: usize = 2;
pub const FP_SHRINK_MOVES: usize = 3;
pub const FP_SHRINK_MOVED: usize = 4;
pub const FP_SHRINK_MOVED_CPU: usize = 5;
pub const FP_SHRINK_MOVED_MEM: usize = 6;
pub const FP_SHRINK_FIRST_FAILED: usize = 7;
pub const FP_SHRINK_WORDS: usize = 8;
pub const FP_REBAL_MOVES: usize = 0;
pub const FP_REBAL_STUCK: usize = 1;
pub const FP_REBAL_STUCK_SKEW: usize = 2;
pub const FP_REBAL_RELAXED: usize = 3;
pub const FP_REBAL_MOVED_CPU: usize = 4;
pub const FP_REBAL_MOVED_MEM: usize = 5;
pub const FP_REBAL_SKEW_BEFORE: usize = 6;
pub const FP_REBAL_SKEW_AFTER: usize = 7;
pub const FP_REBAL_WORDS: usize = 8;
pub const FP_SHRINK_STATE_NEVER: u8 = 0;
pub const FP_SHRINK_STATE_RELEASED: u8 = 1;
pub const FP_SHRINK_STATE_FAILED: u8 = 2;
// the drain sweep under the policy (SPEC.md 2.15): the word indices of a candidate's policy row
pub const FP_DRAIN_STRANDED_SKEW: usize = 0;
pub const FP_DRAIN_RELAXED: usize = 1;
pub const FP_DRAIN_SKEW_BEFORE: usize = 2;
pub const FP_DRAIN_SKEW_AFTER: usize = 3;
pub const FP_DRAIN_POLICY_WORDS: usize = 4;
// the scale-in sweep under the policy (SPEC.md 2.17): the word indices of a variant's policy row
pub const FP_SHRINK_FAILED_SKEW: usize = 0;
pub const FP_SHRINK_RELAXED: usize = 1;
pub const FP_SHRINK_SKEW_BEFORE: usize = 2;
pub const FP_SHRINK_SKEW_AFTER: usize = 3;
pub const FP_SHRINK_POLICY_WORDS: usize = 4;
// scale-out sweep (SPEC.md 2.12): the word indices of a candidate's summary row, and the most new servers
pub const FP_GROW_PENDING: usize = 0;
pub const FP_GROW_PLACED: usize = 1;
pub const FP_GROW_OPENED: usize = 2;
pub const FP_GROW_UNPLACEABLE: usize = 3;
pub const FP_GROW_CAPPED: usize = 4;
pub const FP_GROW_LEFT_CPU: usize = 5;
pub const FP_GROW_LEFT_MEM: usize = 6;
pub const FP_GROW_FIRST_UNPLACED: usize = 7;
pub const FP_GROW_WORDS: usize = 8;
pub const FP_GROW_MAX_NEW: u32 = 8192;
// the scale-out sweep under the policy (SPEC.md 2.18): the word indices of a candidate's policy row
pub const FP_GROW_ON_LIVE: usize = 0;
pub const FP_GROW_RELAXED: usize = 1;
pub const FP_GROW_STUCK_SKEW: usize = 2;
pub const FP_GROW_STUCK_QUOTA: usize = 3;
pub const FP_GROW_SKEW_BEFORE: usize = 4;
pub const FP_GROW_SKEW_AFTER: usize = 5;
pub const FP_GROW_POLICY_WORDS: usize = 8;
// re-planning a running stage (SPEC.md 2.13): enum fp_change, and the word indices of a scenario's summary row
pub const FP_CHANGE_KEPT: u8 = 0;
pub const FP_CHANGE_NEW: u8 = 1;
pub const FP_CHANGE_MOVED: u8 = 2;
pub const FP_CHANGE_LOST: u8 = 3;
pub const FP_CHANGE_ABSENT: u8 = 4;
pub const FP_REPLAN_KEPT: usize = 0;
pub const FP_REPLAN_NEW: usize = 1;
pub const FP_REPLAN_MOVED: usize = 2;
pub const FP_REPLAN_LOST: usize = 3;
pub const FP_REPLAN_ABSENT: usize = 4;
pub const FP_REPLAN_MOVED_CPU: usize = 5;
pub const FP_REPLAN_MOVED_MEM: usize = 6;
pub const FP_REPLAN_WORDS: usize = 8;
pub const FP_K_PLACE: c_int = 0;
pub const FP_K_SORT: c_int = 1;
pub const FP_K_FEAS: c_int = 2;
pub const FP_K_LEVEL: c_int = 3;
pub const FP_K_GEN: c_int = 4;
pub const FP_OPT_AUTO: i64 = -1;
pub const FP_OPT_PIPE_W: c_int = 0;
pub const FP_OPT_PIPE_SEG: c_int = 1;
pub const FP_OPT_PIPE_R: c_int = 2;
pub const FP_OPT_PIPE_LAG: c_int = 3;
pub const FP_OPT_LINK_SLOTS: c_int = 4;
pub const FP_OPT_LINK_BOUNDED: c_int = 5;
pub const FP_OPT_PIPE_FLUSH: c_int = 6;
pub const FP_OPT_SPIN_TICKS: c_int = 7;
pub const FP_OPT_KPACK: c_int = 8;
pub const FP_OPT_SCEN_SORT: c_int = 9;
/// Ignored (kept for ABI stability): the radix path is segmented for S > 1, device-wide for S == 1.
pub const FP_OPT_SEGSORT: c_int = 10;
pub const FP_OPT_SYSTOLIC: c_int = 11;
pub const FP_OPT_LEVELIZE_SYNC: c_int = 12;
pub const FP_OPT_SYSTOLIC_EXTRA: c_int = 13;
pub const FP_OPT_SCREEN: c_int = 14;
pub const FP_OPT_PAYLOAD_LDS: c_int = 15;
pub const FP_OPT_SYSTOLIC_VALU: c_int = 16;
pub const FP_OPT_LINK_PUBLISH: c_int = 17;
pub const FP_OPT_LEVEL_SORT: c_int = 18;
pub const FP_OPT_LEVEL_SMALL: c_int = 19;
pub const FP_OPT_PIPE_PRIO: c_int = 20;
pub const FP_OPT_INDEG_BIN: c_int = 21;
pub const FP_OPT_PACKED: c_int = 22;
pub const FP_OPT_SORT_FUSED: c_int = 23;
pub const FP_OPT_PREPACK: c_int = 24;
pub const FP_GEOM_GROUPS: usize = 0;
pub const FP_GEOM_STAGES: usize = 1;
pub const FP_GEOM_SEGMENTS: usize = 2;
pub const FP_GEOM_RING: usize = 3;
pub const FP_GEOM_LAG: usize = 4;
pub const FP_GEOM_LINK_SLOTS: usize = 5;
pub const FP_GEOM_BOUNDED: usize = 6;
pub const FP_GEOM_RESIDENT: usize = 7;
pub const FP_GEOM_SYSTOLIC: usize = 8;
pub const FP_GEOM_COUNT: usize = 9;

/// Opaque `fp_ctx` (one per host thread; owns a HIP stream on one MI355X).
#[repr(C)]
pub struct fp_ctx {
    _private: [u8; 0],
}

/// depends_on graph as a reversed CSR (row d lists the vertices depending on d).
#[repr(C)]
pub struct fp_graph {
    pub n_vertices: u32,
    pub n_edges: u32,
    pub row_ptr: *const u32,
    pub col: *const u32,
    pub has_deps: *const u8,
}

/// Container requests, SoA.
#[repr(C)]
pub struct fp_containers {
    pub n: u32,
    pub cpu_m: *const u32,
    pub mem_mib: *const u32,
    pub req_labels: *const u32,
    pub conflict: *const u32,
}

/// Node table, SoA, in node-index order; cpu_free/mem_free/conflict_used updated in place.
#[repr(C)]
pub struct fp_nodes {
    pub n: u32,
    pub cpu_free: *mut u32,
    pub mem_free: *mut u32,
    pub labels: *const u32,
    pub conflict_used: *mut u32,
    pub schedulable: *const u8,
}

/// S what-if scenarios, scenario-major arrays ([S][C] containers, [S][N] nodes).
#[repr(C)]
pub struct fp_batch {
    pub n_scen: u32,
    pub scen_base: u32,
    pub n_containers: u32,
    pub n_nodes: u32,
    pub cpu_m: *const u32,
    pub mem_mib: *const u32,
    pub req_labels: *const u32,
    pub conflict: *const u32,
    pub level: *const u32,
    pub cpu_free: *mut u32,
    pub mem_free: *mut u32,
    pub labels: *const u32,
    pub conflict_used: *mut u32,
    pub schedulable: *const u8,
    pub assign: *mut u32,
    pub reason: *mut u8,
    pub cost: *mut u64,
}

#[link(name = "fleetplace")]
unsafe extern "C" {
    pub fn fp_ctx_create(out: *mut *mut fp_ctx, device: c_int) -> c_int;
    pub fn fp_ctx_destroy(ctx: *mut fp_ctx);
    pub fn fp_ctx_set_stream(ctx: *mut fp_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn fp_ctx_reset_stream(ctx: *mut fp_ctx) -> c_int;
    pub fn fp_ctx_sync(ctx: *mut fp_ctx) -> c_int;
    pub fn fp_strerror(code: c_int) -> *const c_char;
    pub fn fp_abi_version() -> c_int;
    pub fn fp_ctx_profile(ctx: *mut fp_ctx, enable: c_int) -> c_int;
    pub fn fp_ctx_kernel_stats(ctx: *mut fp_ctx, kernel_id: c_int, total_ms: *mut f64, launches: *mut u64) -> c_int;
    pub fn fp_ctx_place_path(ctx: *mut fp_ctx, out3: *mut u32) -> c_int;
    pub fn fp_ctx_set_option(ctx: *mut fp_ctx, option: c_int, value: i64) -> c_int;
    pub fn fp_ctx_get_option(ctx: *mut fp_ctx, option: c_int, value: *mut i64) -> c_int;

    pub fn fp_legacy_order(ctx: *mut fp_ctx, g: *const fp_graph, perm_out: *mut u32) -> c_int;
    pub fn fp_levelize(ctx: *mut fp_ctx, g: *const fp_graph, level_out: *mut u32, order_out: *mut u32,
                       n_cycle_out: *mut u32) -> c_int;
    pub fn fp_place(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                    assign_out: *mut u32, reason_out: *mut u8) -> c_int;
    pub fn fp_place_batch(ctx: *mut fp_ctx, b: *const fp_batch) -> c_int;
    pub fn fp_place_policy(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                           strategy: u32, preferred_labels: u32, node_count: *mut u32, assign_out: *mut u32,
                           reason_out: *mut u8) -> c_int;
    pub fn fp_place_batch_policy(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                 preferred_labels: *const u32, node_count: *mut u32) -> c_int;
    pub fn fp_dev_place_batch_policy(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                     preferred_labels: *const u32, node_count: *mut u32) -> c_int;
    pub fn fp_place_policy_spread(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                                  strategy: u32, preferred_labels: u32, node_count: *mut u32, domain: *const u32,
                                  max_skew: u32, assign_out: *mut u32, reason_out: *mut u8) -> c_int;
    pub fn fp_place_batch_policy_spread(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                        preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                        max_skew: *const u32) -> c_int;
    pub fn fp_place_policy_fallback(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                                    strategy: u32, preferred_labels: u32, node_count: *mut u32, domain: *const u32,
                                    max_skew: u32, relax_mask: *const u32, n_hops: u32, assign_out: *mut u32,
                                    reason_out: *mut u8, hops_out: *mut u8) -> c_int;
    pub fn fp_place_batch_policy_fallback(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                          preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                          max_skew: *const u32, relax_mask: *const u32, n_hops: *const u32,
                                          hops_out: *mut u8) -> c_int;
    pub fn fp_place_policy_quota(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                                 strategy: u32, preferred_labels: u32, node_count: *mut u32, domain: *const u32,
                                 max_skew: u32, relax_mask: *const u32, n_hops: u32, assign_out: *mut u32,
                                 reason_out: *mut u8, hops_out: *mut u8, quota: *const u32, quota_used: *mut u32,
                                 quota_why_out: *mut u8) -> c_int;
    pub fn fp_place_batch_policy_quota(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                       preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                       max_skew: *const u32, relax_mask: *const u32, n_hops: *const u32,
                                       hops_out: *mut u8, quota: *const u32, quota_used: *mut u32,
                                       quota_why_out: *mut u8) -> c_int;
    pub fn fp_feasibility(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes, first_out: *mut u32,
                          count_out: *mut u32, bitmap_out: *mut u64) -> c_int;
    pub fn fp_explain(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes, sel: *const u32, n_sel: u32,
                      ignore_labels: u32, rows_out: *mut u32) -> c_int;
    pub fn fp_explain_batch(ctx: *mut fp_ctx, b: *const fp_batch, reason_mask: u32, ignore_labels: *const u32,
                            hist_out: *mut u32) -> c_int;
    pub fn fp_drain_sweep(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes, assign: *const u32,
                          group: *const u32, n_cand: u32, strategy: u32, preferred_labels: u32,
                          node_count: *const u32, assign_out: *mut u32, reason_out: *mut u8,
                          summary_out: *mut u32) -> c_int;
    pub fn fp_drain_sweep_policy(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                                 assign: *const u32, group: *const u32, n_cand: u32, strategy: u32,
                                 preferred_labels: u32, node_count: *const u32, domain: *const u32, max_skew: u32,
                                 relax_mask: *const u32, n_hops: u32, assign_out: *mut u32, reason_out: *mut u8,
                                 hops_out: *mut u8, summary_out: *mut u32, policy_out: *mut u32) -> c_int;
    pub fn fp_shrink_sweep(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes, assign: *const u32,
                           try_order: *const u32, n_var: u32, n_try: u32, strategy: u32, preferred_labels: u32,
                           node_count: *const u32, assign_out: *mut u32, state_out: *mut u8, blocker_out: *mut u32,
                           summary_out: *mut u32) -> c_int;
    pub fn fp_shrink_sweep_policy(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                                  assign: *const u32, try_order: *const u32, n_var: u32, n_try: u32, strategy: u32,
                                  preferred_labels: u32, node_count: *const u32, domain: *const u32, max_skew: u32,
                                  relax_mask: *const u32, n_hops: u32, assign_out: *mut u32, state_out: *mut u8,
                                  blocker_out: *mut u32, summary_out: *mut u32, hops_out: *mut u8,
                                  blocker_reason_out: *mut u8, policy_out: *mut u32) -> c_int;
    pub fn fp_rebalance_sweep(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                              assign: *const u32, victim_order: *const u32, n_var: u32, n_try: u32,
                              max_moves: *const u32, strategy: u32, preferred_labels: u32, node_count: *const u32,
                              domain: *const u32, max_skew: u32, relax_mask: *const u32, n_hops: u32,
                              assign_out: *mut u32, hops_out: *mut u8, reason_out: *mut u8,
                              summary_out: *mut u32) -> c_int;
    pub fn fp_grow_sweep(ctx: *mut fp_ctx, c: *const fp_containers, reason: *const u8, reason_mask: u32, n_cand: u32,
                         t_cpu: *const u32, t_mem: *const u32, t_labels: *const u32, t_max: *const u32,
                         max_new: u32, summary_out: *mut u32, assign_out: *mut u32) -> c_int;
    pub fn fp_grow_sweep_policy(ctx: *mut fp_ctx, c: *const fp_containers, reason: *const u8, reason_mask: u32,
                                nodes: *const fp_nodes, node_count: *const u32, n_cand: u32, t_cpu: *const u32,
                                t_mem: *const u32, t_labels: *const u32, t_max: *const u32, max_new: u32,
                                strategy: u32, preferred_labels: u32, domain: *const u32, t_domain: *const u32,
                                max_skew: u32, relax_mask: *const u32, n_hops: u32, quota: *const u32,
                                quota_used: *const u32, summary_out: *mut u32, policy_out: *mut u32,
                                assign_out: *mut u32, hops_out: *mut u8, reason_out: *mut u8) -> c_int;
    pub fn fp_replan(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                     prev: *const u32, strategy: u32, preferred_labels: u32, node_count: *mut u32,
                     assign_out: *mut u32, reason_out: *mut u8, change_out: *mut u8, summary_out: *mut u32) -> c_int;
    pub fn fp_replan_batch(ctx: *mut fp_ctx, b: *const fp_batch, prev: *const u32, strategy: *const u32,
                           preferred_labels: *const u32, node_count: *mut u32, change_out: *mut u8,
                           summary_out: *mut u32) -> c_int;
    pub fn fp_replan_policy(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *mut fp_nodes, level: *const u32,
                            prev: *const u32, strategy: u32, preferred_labels: u32, node_count: *mut u32,
                            domain: *const u32, max_skew: u32, relax_mask: *const u32, n_hops: u32,
                            assign_out: *mut u32, reason_out: *mut u8, hops_out: *mut u8, quota: *const u32,
                            quota_used: *mut u32, quota_why_out: *mut u8, change_out: *mut u8,
                            summary_out: *mut u32) -> c_int;
    pub fn fp_replan_batch_policy(ctx: *mut fp_ctx, b: *const fp_batch, prev: *const u32, strategy: *const u32,
                                  preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                  max_skew: *const u32, relax_mask: *const u32, n_hops: *const u32,
                                  hops_out: *mut u8, quota: *const u32, quota_used: *mut u32,
                                  quota_why_out: *mut u8, change_out: *mut u8, summary_out: *mut u32) -> c_int;
    pub fn fp_plan_stage(ctx: *mut fp_ctx, g: *const fp_graph, c: *const fp_containers, nodes: *mut fp_nodes,
                         perm_out: *mut u32, level_out: *mut u32, order_out: *mut u32, n_cycle_out: *mut u32,
                         first_out: *mut u32, count_out: *mut u32, assign_out: *mut u32, reason_out: *mut u8)
                         -> c_int;

    pub fn fp_dev_legacy_order(ctx: *mut fp_ctx, g: *const fp_graph, perm_out: *mut u32) -> c_int;
    pub fn fp_dev_levelize(ctx: *mut fp_ctx, g: *const fp_graph, level_out: *mut u32, order_out: *mut u32,
                           n_cycle_out_dev: *mut u32) -> c_int;
    pub fn fp_dev_place_batch(ctx: *mut fp_ctx, b: *const fp_batch) -> c_int;
    pub fn fp_place_ws_bytes(ctx: *mut fp_ctx, n_scen: u32, n_containers: u32, n_nodes: u32,
                             bytes_out: *mut u64) -> c_int;
    pub fn fp_place_geometry(ctx: *mut fp_ctx, n_scen: u32, n_containers: u32, n_nodes: u32,
                             out: *mut u32) -> c_int;
    pub fn fp_dev_feasibility(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                              first_out: *mut u32, count_out: *mut u32, bitmap_out: *mut u64) -> c_int;
    pub fn fp_dev_feasibility_batch(ctx: *mut fp_ctx, b: *const fp_batch, first_out: *mut u32,
                                    count_out: *mut u32) -> c_int;
    pub fn fp_dev_explain(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes, sel: *const u32,
                          n_sel: u32, ignore_labels: u32, rows_out: *mut u32) -> c_int;
    pub fn fp_dev_explain_batch(ctx: *mut fp_ctx, b: *const fp_batch, reason_mask: u32, ignore_labels: *const u32,
                                hist_out: *mut u32) -> c_int;
    pub fn fp_dev_place_batch_policy_spread(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                            preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                            max_skew: *const u32) -> c_int;
    pub fn fp_dev_place_batch_policy_fallback(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                              preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                              max_skew: *const u32, relax_mask: *const u32, n_hops: *const u32,
                                              hops_out: *mut u8) -> c_int;
    pub fn fp_dev_place_batch_policy_quota(ctx: *mut fp_ctx, b: *const fp_batch, strategy: *const u32,
                                           preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                           max_skew: *const u32, relax_mask: *const u32, n_hops: *const u32,
                                           hops_out: *mut u8, quota: *const u32, quota_used: *mut u32,
                                           quota_why_out: *mut u8) -> c_int;
    pub fn fp_dev_drain_sweep(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes, assign: *const u32,
                              group: *const u32, n_cand: u32, strategy: u32, preferred_labels: u32,
                              node_count: *const u32, assign_out: *mut u32, reason_out: *mut u8,
                              summary_out: *mut u32) -> c_int;
    // relax_mask is a HOST array here too: the one exception to "fp_dev_* take device pointers"
    pub fn fp_dev_drain_sweep_policy(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                                     assign: *const u32, group: *const u32, n_cand: u32, strategy: u32,
                                     preferred_labels: u32, node_count: *const u32, domain: *const u32,
                                     max_skew: u32, relax_mask: *const u32, n_hops: u32, assign_out: *mut u32,
                                     reason_out: *mut u8, hops_out: *mut u8, summary_out: *mut u32,
                                     policy_out: *mut u32) -> c_int;
    pub fn fp_dev_shrink_sweep(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                               assign: *const u32, try_order: *const u32, n_var: u32, n_try: u32, strategy: u32,
                               preferred_labels: u32, node_count: *const u32, assign_out: *mut u32,
                               state_out: *mut u8, blocker_out: *mut u32, summary_out: *mut u32) -> c_int;
    pub fn fp_dev_shrink_sweep_policy(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                                      assign: *const u32, try_order: *const u32, n_var: u32, n_try: u32,
                                      strategy: u32, preferred_labels: u32, node_count: *const u32,
                                      domain: *const u32, max_skew: u32, relax_mask: *const u32, n_hops: u32,
                                      assign_out: *mut u32, state_out: *mut u8, blocker_out: *mut u32,
                                      summary_out: *mut u32, hops_out: *mut u8, blocker_reason_out: *mut u8,
                                      policy_out: *mut u32) -> c_int;
    pub fn fp_dev_rebalance_sweep(ctx: *mut fp_ctx, c: *const fp_containers, nodes: *const fp_nodes,
                              assign: *const u32, victim_order: *const u32, n_var: u32, n_try: u32,
                              max_moves: *const u32, strategy: u32, preferred_labels: u32, node_count: *const u32,
                              domain: *const u32, max_skew: u32, relax_mask: *const u32, n_hops: u32,
                              assign_out: *mut u32, hops_out: *mut u8, reason_out: *mut u8,
                              summary_out: *mut u32) -> c_int;
    pub fn fp_dev_grow_sweep(ctx: *mut fp_ctx, c: *const fp_containers, reason: *const u8, reason_mask: u32,
                             n_cand: u32, t_cpu: *const u32, t_mem: *const u32, t_labels: *const u32,
                             t_max: *const u32, max_new: u32, summary_out: *mut u32, assign_out: *mut u32) -> c_int;
    pub fn fp_dev_grow_sweep_policy(ctx: *mut fp_ctx, c: *const fp_containers, reason: *const u8, reason_mask: u32,
                                    nodes: *const fp_nodes, node_count: *const u32, n_cand: u32, t_cpu: *const u32,
                                    t_mem: *const u32, t_labels: *const u32, t_max: *const u32, max_new: u32,
                                    strategy: u32, preferred_labels: u32, domain: *const u32, t_domain: *const u32,
                                    max_skew: u32, relax_mask: *const u32, n_hops: u32, quota: *const u32,
                                    quota_used: *const u32, summary_out: *mut u32, policy_out: *mut u32,
                                    assign_out: *mut u32, hops_out: *mut u8, reason_out: *mut u8) -> c_int;
    pub fn fp_dev_replan_batch(ctx: *mut fp_ctx, b: *const fp_batch, prev: *const u32, strategy: *const u32,
                               preferred_labels: *const u32, node_count: *mut u32, change_out: *mut u8,
                               summary_out: *mut u32) -> c_int;
    pub fn fp_dev_replan_batch_policy(ctx: *mut fp_ctx, b: *const fp_batch, prev: *const u32, strategy: *const u32,
                                      preferred_labels: *const u32, node_count: *mut u32, domain: *const u32,
                                      max_skew: *const u32, relax_mask: *const u32, n_hops: *const u32,
                                      hops_out: *mut u8, quota: *const u32, quota_used: *mut u32,
                                      quota_why_out: *mut u8, change_out: *mut u8, summary_out: *mut u32) -> c_int;
    pub fn fp_dev_argmin_cost(ctx: *mut fp_ctx, cost: *const u64, n: u32, best_dev: *mut u32) -> c_int;
    pub fn fp_dev_gen_batch(ctx: *mut fp_ctx, seed: u64, b: *const fp_batch, flags: u32) -> c_int;
}
