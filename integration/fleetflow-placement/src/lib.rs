//! fleetflow-placement: FleetFlow's plan path on an MI355X (HIP/gfx950, libfleetplace.so).
//!
//! Drop-in replacements for the three seams of the reference:
//! * [`order_by_dependencies`] -- same signature and output as
//!   `fleetflow_container::order_by_dependencies` (crates/fleetflow-container/src/engine.rs:64-85),
//!   for the call at engine.rs:157;
//! * [`start_levels`] / [`start_waves`] -- Kahn start levels, the parallel start waves for
//!   `DeployEngine::create_and_start` (engine.rs:355-452);
//! * [`resolve_target_server`] -- the server choice of
//!   crates/fleetflow-controlplane/src/handlers/deploy.rs:390-398 (`servers.first()`), exactly
//!   as the reference computes it (no planning involved, no GPU needed), and
//!   [`Planner::place`] / [`place_stage`] -- the first-fit-decreasing fan-out that replaces it
//!   when server capacity matters;
//! * [`plan_scenarios`] / [`Planner::place_batch`] -- what-if planning: many independent
//!   scenarios in one call, a packed cost per scenario and the best plan, the single-host
//!   counterpart of the controlplane routing a deploy to one target (deploy.rs:441-451).
//!
//! Strings never cross the ABI: names map to u32 ids in stage order here.  There is no CPU
//! fallback for the planning calls: without an MI355X they return [`PlanError`] (FP_EDEVICE),
//! and [`order_by_dependencies`] panics like any use of the crate on a host without the GPU
//! it is built for.
pub mod ffi;

use fleetflow_core::Flow;
use std::cell::RefCell;
use std::collections::HashMap;
use std::ffi::CStr;
use std::fmt;

/// A negative FP_E* code from libfleetplace.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct PlanError(pub i32);

impl fmt::Display for PlanError {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        let msg = unsafe { CStr::from_ptr(ffi::fp_strerror(self.0)) };
        write!(f, "fleetplace: {} ({})", msg.to_string_lossy(), self.0)
    }
}
impl std::error::Error for PlanError {}

fn check(rc: i32) -> Result<(), PlanError> {
    if rc == ffi::FP_OK { Ok(()) } else { Err(PlanError(rc)) }
}

/// One planner context: a HIP stream on one MI355X.  Not shared between threads
/// (fleetplace.h: one fp_ctx per host thread); [`with_planner`] keeps one per thread.
pub struct Planner {
    ctx: *mut ffi::fp_ctx,
}

impl Planner {
    pub fn new(device: i32) -> Result<Self, PlanError> {
        let mut ctx = std::ptr::null_mut();
        check(unsafe { ffi::fp_ctx_create(&mut ctx, device) })?;
        Ok(Planner { ctx })
    }

    /// engine.rs:67-85 on indices: `has_deps[i]` = known in flow.services AND depends_on
    /// non-empty; returns the stable two-bucket permutation.
    pub fn legacy_order(&mut self, has_deps: &[u8]) -> Result<Vec<u32>, PlanError> {
        let g = ffi::fp_graph { n_vertices: has_deps.len() as u32, n_edges: 0, row_ptr: std::ptr::null(),
                                col: std::ptr::null(), has_deps: has_deps.as_ptr() };
        let mut perm = vec![0u32; has_deps.len()];
        check(unsafe { ffi::fp_legacy_order(self.ctx, &g, perm.as_mut_ptr()) })?;
        Ok(perm)
    }

    /// Kahn levels of a reversed CSR (SPEC.md 2.2): (level per vertex, FP_NONE on/after a
    /// cycle; order by (level, index); number of cycle vertices).
    pub fn levelize(&mut self, row_ptr: &[u32], col: &[u32], has_deps: &[u8])
                    -> Result<(Vec<u32>, Vec<u32>, u32), PlanError> {
        let v = has_deps.len();
        if v > 0 && row_ptr.len() != v + 1 {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let g = ffi::fp_graph { n_vertices: v as u32, n_edges: col.len() as u32, row_ptr: row_ptr.as_ptr(),
                                col: if col.is_empty() { std::ptr::null() } else { col.as_ptr() },
                                has_deps: has_deps.as_ptr() };
        let (mut level, mut order, mut ncyc) = (vec![0u32; v], vec![0u32; v], 0u32);
        check(unsafe { ffi::fp_levelize(self.ctx, &g, level.as_mut_ptr(), order.as_mut_ptr(), &mut ncyc) })?;
        Ok((level, order, ncyc))
    }

    /// First-fit-decreasing placement (SPEC.md 2.3); `nodes` is updated in place.
    /// Returns (assign per container, FP_NONE if unplaced; reason per container).
    pub fn place(&mut self, c: &Containers, nodes: &mut Nodes, level: Option<&[u32]>)
                 -> Result<(Vec<u32>, Vec<u8>), PlanError> {
        let n = c.cpu_m.len();
        // fp_place reads every container array for n elements and reads / writes every node
        // array for nodes.len(): a shorter Vec would be read out of bounds from safe code
        if !c.all_len(n) || !nodes.all_len(nodes.cpu_free.len()) || level.map_or(false, |l| l.len() != n) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut ns = ffi::fp_nodes { n: nodes.cpu_free.len() as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                     mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                     conflict_used: nodes.conflict_used.as_mut_ptr(),
                                     schedulable: nodes.schedulable.as_ptr() };
        let (mut assign, mut reason) = (vec![0u32; n], vec![0u8; n]);
        check(unsafe {
            ffi::fp_place(self.ctx, &cs, &mut ns, level.map_or(std::ptr::null(), |l| l.as_ptr()),
                          assign.as_mut_ptr(), reason.as_mut_ptr())
        })?;
        Ok((assign, reason))
    }

    /// Rejection diagnosis (SPEC.md 2.9, fleetplace.h `fp_explain`): one row of `ffi::FP_EXPLAIN_WORDS`
    /// words per container of `sel` (None = every container in order) on the node table `nodes`, which is
    /// not changed; `ignore_labels` are the required-label bits given up.  Word indices: `ffi::FP_EXPLAIN_*`.
    pub fn explain(&mut self, c: &Containers, nodes: &Nodes, sel: Option<&[u32]>, ignore_labels: u32)
                   -> Result<Vec<[u32; ffi::FP_EXPLAIN_WORDS]>, PlanError> {
        let n = c.cpu_m.len();
        if !c.all_len(n) || !nodes.all_len(nodes.cpu_free.len()) || sel.map_or(false, |s| s.iter().any(|&i| i as usize >= n)) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // fp_explain reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nodes.cpu_free.len() as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let m = sel.map_or(n, |s| s.len());
        let mut rows = vec![[0u32; ffi::FP_EXPLAIN_WORDS]; m];
        check(unsafe {
            ffi::fp_explain(self.ctx, &cs, &ns, sel.map_or(std::ptr::null(), |s| s.as_ptr()), m as u32, ignore_labels,
                            rows.as_mut_ptr() as *mut u32)
        })?;
        Ok(rows)
    }

    /// Drain what-if sweep (SPEC.md 2.11, fleetplace.h `fp_drain_sweep`): `nodes` is the live table, `assign`
    /// the node each container runs on (`ffi::FP_NONE` = not running), `group` the candidate of each node
    /// (< `n_cand`, `ffi::FP_NONE` = none).  Every candidate's evictees are re-placed, independently and from
    /// the same base state, under `strategy` / `preferred_labels`; no input is changed.  Returns (the new node
    /// per container, the reason per container, one row of `ffi::FP_DRAIN_WORDS` words per candidate).
    #[allow(clippy::too_many_arguments)]
    pub fn drain_sweep(&mut self, c: &Containers, nodes: &Nodes, assign: &[u32], group: &[u32], n_cand: u32,
                       strategy: u32, preferred_labels: u32, node_count: Option<&[u32]>)
                       -> Result<(Vec<u32>, Vec<u8>, Vec<[u32; ffi::FP_DRAIN_WORDS]>), PlanError> {
        let (n, nn) = (c.cpu_m.len(), nodes.cpu_free.len());
        if !c.all_len(n) || !nodes.all_len(nn) || assign.len() != n || group.len() != nn
            || node_count.map_or(false, |k| k.len() != nn) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // fp_drain_sweep reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let (mut out, mut reason) = (vec![0u32; n], vec![0u8; n]);
        let mut rows = vec![[0u32; ffi::FP_DRAIN_WORDS]; n_cand as usize];
        check(unsafe {
            ffi::fp_drain_sweep(self.ctx, &cs, &ns, assign.as_ptr(), group.as_ptr(), n_cand, strategy, preferred_labels,
                                node_count.map_or(std::ptr::null(), |k| k.as_ptr()), out.as_mut_ptr(),
                                reason.as_mut_ptr(), rows.as_mut_ptr() as *mut u32)
        })?;
        Ok((out, reason, rows))
    }

    /// Scale-in sweep (SPEC.md 2.16, fleetplace.h `fp_shrink_sweep`): `nodes` is the live table, `assign` the
    /// node each container runs on, `try_order` one release order per variant, `n_try` entries each
    /// (`ffi::FP_NONE` entries are skipped).  Every variant tries its nodes in order from the same base state; an
    /// attempt whose containers all find another node releases its node, any other is undone.  No input is
    /// changed.  Returns per variant (the final node per container, the state per node (`ffi::FP_SHRINK_STATE_*`),
    /// the blocker per node, its row of `ffi::FP_SHRINK_WORDS` words).
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn shrink_sweep(&mut self, c: &Containers, nodes: &Nodes, assign: &[u32], try_order: &[u32], n_try: u32,
                        strategy: u32, preferred_labels: u32, node_count: Option<&[u32]>)
                        -> Result<(Vec<u32>, Vec<u8>, Vec<u32>, Vec<[u32; ffi::FP_SHRINK_WORDS]>), PlanError> {
        let (n, nn) = (c.cpu_m.len(), nodes.cpu_free.len());
        let n_var = if n_try == 0 { 0 } else { try_order.len() / n_try as usize };
        if !c.all_len(n) || !nodes.all_len(nn) || assign.len() != n || try_order.len() != n_var * n_try as usize
            || n_var > u32::MAX as usize || node_count.map_or(false, |k| k.len() != nn) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // fp_shrink_sweep reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let (mut out, mut state, mut blocker) = (vec![0u32; n_var * n], vec![0u8; n_var * nn], vec![0u32; n_var * nn]);
        let mut rows = vec![[0u32; ffi::FP_SHRINK_WORDS]; n_var];
        check(unsafe {
            ffi::fp_shrink_sweep(self.ctx, &cs, &ns, assign.as_ptr(), try_order.as_ptr(), n_var as u32, n_try, strategy,
                                 preferred_labels, node_count.map_or(std::ptr::null(), |k| k.as_ptr()),
                                 out.as_mut_ptr(), state.as_mut_ptr(), blocker.as_mut_ptr(),
                                 rows.as_mut_ptr() as *mut u32)
        })?;
        Ok((out, state, blocker, rows))
    }

    /// The scale-in sweep under the policy (SPEC.md 2.17, fleetplace.h `fp_shrink_sweep_policy`): `shrink_sweep`
    /// with every move held to the spread constraint (`domain` ids below `ffi::FP_SPREAD_MAX_DOMAINS` and
    /// `max_skew`; None or 0 = none) and the fallback chain (`relax_mask`: per hop the label bits it gives up, at
    /// most `ffi::FP_FALLBACK_MAX_HOPS`; empty = none), and every release to the bound rule.  Returns per variant
    /// (the final node and the hop of the last move per container, the state, the blocker and the blocker's
    /// reason per node, its row of `ffi::FP_SHRINK_WORDS` and its row of `ffi::FP_SHRINK_POLICY_WORDS` words).
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn shrink_sweep_policy(&mut self, c: &Containers, nodes: &Nodes, assign: &[u32], try_order: &[u32], n_try: u32,
                               strategy: u32, preferred_labels: u32, node_count: Option<&[u32]>,
                               domain: Option<&[u32]>, max_skew: u32, relax_mask: &[u32])
                               -> Result<(Vec<u32>, Vec<u8>, Vec<u8>, Vec<u32>, Vec<u8>, Vec<[u32; ffi::FP_SHRINK_WORDS]>,
                                          Vec<[u32; ffi::FP_SHRINK_POLICY_WORDS]>), PlanError> {
        let (n, nn) = (c.cpu_m.len(), nodes.cpu_free.len());
        let n_var = if n_try == 0 { 0 } else { try_order.len() / n_try as usize };
        if !c.all_len(n) || !nodes.all_len(nn) || assign.len() != n || try_order.len() != n_var * n_try as usize
            || n_var > u32::MAX as usize || node_count.map_or(false, |k| k.len() != nn)
            || domain.map_or(false, |d| d.len() != nn) || relax_mask.len() > ffi::FP_FALLBACK_MAX_HOPS as usize {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // the sweep reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let (mut out, mut state, mut blocker) = (vec![0u32; n_var * n], vec![0u8; n_var * nn], vec![0u32; n_var * nn]);
        let (mut hops, mut why) = (vec![0u8; n_var * n], vec![0u8; n_var * nn]);
        let mut rows = vec![[0u32; ffi::FP_SHRINK_WORDS]; n_var];
        let mut prows = vec![[0u32; ffi::FP_SHRINK_POLICY_WORDS]; n_var];
        check(unsafe {
            ffi::fp_shrink_sweep_policy(self.ctx, &cs, &ns, assign.as_ptr(), try_order.as_ptr(), n_var as u32, n_try,
                                        strategy, preferred_labels, node_count.map_or(std::ptr::null(), |k| k.as_ptr()),
                                        domain.map_or(std::ptr::null(), |d| d.as_ptr()), max_skew,
                                        if relax_mask.is_empty() { std::ptr::null() } else { relax_mask.as_ptr() },
                                        relax_mask.len() as u32, out.as_mut_ptr(), state.as_mut_ptr(),
                                        blocker.as_mut_ptr(), rows.as_mut_ptr() as *mut u32, hops.as_mut_ptr(),
                                        why.as_mut_ptr(), prows.as_mut_ptr() as *mut u32)
        })?;
        Ok((out, hops, state, blocker, why, rows, prows))
    }

    /// Rebalance sweep (SPEC.md 2.19, fleetplace.h `fp_rebalance_sweep`): variant v visits the containers of
    /// `victim_order[v * n_try ..][.. n_try]` (`ffi::FP_NONE` entries are skipped) and lifts every one whose node
    /// lies in a heavy domain (eligible, count - min > `max_skew`) off its node, to place it as the only container
    /// of a `fp_place_policy_fallback` call; a rejected attempt leaves the state as it was.  `max_moves`: the move
    /// budget per variant (None or `ffi::FP_NONE` = unlimited); `node_count` None means derived from `assign`.
    /// Returns per variant (the final node, the hop of the move and the reason of a rejected last attempt per
    /// container, and its row of `ffi::FP_REBAL_WORDS` words).
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn rebalance_sweep(&mut self, c: &Containers, nodes: &Nodes, assign: &[u32], victim_order: &[u32], n_try: u32,
                           max_moves: Option<&[u32]>, strategy: u32, preferred_labels: u32,
                           node_count: Option<&[u32]>, domain: Option<&[u32]>, max_skew: u32, relax_mask: &[u32])
                           -> Result<(Vec<u32>, Vec<u8>, Vec<u8>, Vec<[u32; ffi::FP_REBAL_WORDS]>), PlanError> {
        let (n, nn) = (c.cpu_m.len(), nodes.cpu_free.len());
        let n_var = if n_try == 0 { 0 } else { victim_order.len() / n_try as usize };
        if !c.all_len(n) || !nodes.all_len(nn) || assign.len() != n || victim_order.len() != n_var * n_try as usize
            || n_var > u32::MAX as usize || max_moves.map_or(false, |m| m.len() != n_var)
            || node_count.map_or(false, |k| k.len() != nn) || domain.map_or(false, |d| d.len() != nn)
            || relax_mask.len() > ffi::FP_FALLBACK_MAX_HOPS as usize {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // the sweep reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let (mut out, mut hops, mut why) = (vec![0u32; n_var * n], vec![0u8; n_var * n], vec![0u8; n_var * n]);
        let mut rows = vec![[0u32; ffi::FP_REBAL_WORDS]; n_var];
        check(unsafe {
            ffi::fp_rebalance_sweep(self.ctx, &cs, &ns, assign.as_ptr(), victim_order.as_ptr(), n_var as u32, n_try,
                                    max_moves.map_or(std::ptr::null(), |m| m.as_ptr()), strategy, preferred_labels,
                                    node_count.map_or(std::ptr::null(), |k| k.as_ptr()),
                                    domain.map_or(std::ptr::null(), |d| d.as_ptr()), max_skew,
                                    if relax_mask.is_empty() { std::ptr::null() } else { relax_mask.as_ptr() },
                                    relax_mask.len() as u32, out.as_mut_ptr(), hops.as_mut_ptr(), why.as_mut_ptr(),
                                    rows.as_mut_ptr() as *mut u32)
        })?;
        Ok((out, hops, why, rows))
    }

    /// The drain sweep under the policy (SPEC.md 2.15, fleetplace.h `fp_drain_sweep_policy`): `drain_sweep` with
    /// every move held to the spread constraint (`domain` ids below `ffi::FP_SPREAD_MAX_DOMAINS` and `max_skew`;
    /// None or 0 = none) and the fallback chain (`relax_mask`: per hop the label bits it gives up, at most
    /// `ffi::FP_FALLBACK_MAX_HOPS`; empty = none).  Each candidate's domain counts leave its own nodes out.
    /// Returns (the new node, the reason and the hop per container, one row of `ffi::FP_DRAIN_WORDS` and one of
    /// `ffi::FP_DRAIN_POLICY_WORDS` words per candidate).
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn drain_sweep_policy(&mut self, c: &Containers, nodes: &Nodes, assign: &[u32], group: &[u32], n_cand: u32,
                              strategy: u32, preferred_labels: u32, node_count: Option<&[u32]>,
                              domain: Option<&[u32]>, max_skew: u32, relax_mask: &[u32])
                              -> Result<(Vec<u32>, Vec<u8>, Vec<u8>, Vec<[u32; ffi::FP_DRAIN_WORDS]>,
                                         Vec<[u32; ffi::FP_DRAIN_POLICY_WORDS]>), PlanError> {
        let (n, nn) = (c.cpu_m.len(), nodes.cpu_free.len());
        if !c.all_len(n) || !nodes.all_len(nn) || assign.len() != n || group.len() != nn
            || node_count.map_or(false, |k| k.len() != nn) || domain.map_or(false, |d| d.len() != nn)
            || relax_mask.len() > ffi::FP_FALLBACK_MAX_HOPS as usize {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // the sweep reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let (mut out, mut reason, mut hops) = (vec![0u32; n], vec![0u8; n], vec![0u8; n]);
        let mut rows = vec![[0u32; ffi::FP_DRAIN_WORDS]; n_cand as usize];
        let mut prows = vec![[0u32; ffi::FP_DRAIN_POLICY_WORDS]; n_cand as usize];
        check(unsafe {
            ffi::fp_drain_sweep_policy(self.ctx, &cs, &ns, assign.as_ptr(), group.as_ptr(), n_cand, strategy,
                                       preferred_labels, node_count.map_or(std::ptr::null(), |k| k.as_ptr()),
                                       domain.map_or(std::ptr::null(), |d| d.as_ptr()), max_skew,
                                       if relax_mask.is_empty() { std::ptr::null() } else { relax_mask.as_ptr() },
                                       relax_mask.len() as u32, out.as_mut_ptr(), reason.as_mut_ptr(),
                                       hops.as_mut_ptr(), rows.as_mut_ptr() as *mut u32,
                                       prows.as_mut_ptr() as *mut u32)
        })?;
        Ok((out, reason, hops, rows, prows))
    }

    /// Scale-out sweep (SPEC.md 2.12, fleetplace.h `fp_grow_sweep`): the pending containers are those whose
    /// `reason` has its bit set in `reason_mask` (0 = every container, `reason` may be None); candidate k is a
    /// server template (`t_cpu[k]`, `t_mem[k]`, `t_labels[k]`) of which at most `t_max[k]` (None = `max_new`
    /// <= `ffi::FP_GROW_MAX_NEW`) are opened, first fit.  No input is changed.  Returns one row of
    /// `ffi::FP_GROW_WORDS` words per candidate and, with `want_assign`, the ordinal of the new server per
    /// candidate and container (`ffi::FP_NONE` = none), candidate-major.
    #[allow(clippy::too_many_arguments)]
    pub fn grow_sweep(&mut self, c: &Containers, reason: Option<&[u8]>, reason_mask: u32, t_cpu: &[u32], t_mem: &[u32],
                      t_labels: &[u32], t_max: Option<&[u32]>, max_new: u32, want_assign: bool)
                      -> Result<(Vec<[u32; ffi::FP_GROW_WORDS]>, Option<Vec<u32>>), PlanError> {
        let (n, k) = (c.cpu_m.len(), t_cpu.len());
        if !c.all_len(n) || t_mem.len() != k || t_labels.len() != k || t_max.map_or(false, |m| m.len() != k)
            || (reason_mask != 0 && reason.map_or(true, |r| r.len() != n)) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut rows = vec![[0u32; ffi::FP_GROW_WORDS]; k];
        let mut assign = if want_assign { Some(vec![ffi::FP_NONE; k * n]) } else { None };
        let reason_ptr = if reason_mask != 0 { reason.map_or(std::ptr::null(), |r| r.as_ptr()) } else { std::ptr::null() };
        check(unsafe {
            ffi::fp_grow_sweep(self.ctx, &cs, reason_ptr, reason_mask, k as u32, t_cpu.as_ptr(), t_mem.as_ptr(),
                               t_labels.as_ptr(), t_max.map_or(std::ptr::null(), |m| m.as_ptr()), max_new,
                               rows.as_mut_ptr() as *mut u32,
                               assign.as_mut().map_or(std::ptr::null_mut(), |a| a.as_mut_ptr()))
        })?;
        Ok((rows, assign))
    }

    /// The scale-out sweep under the policy (SPEC.md 2.18, fleetplace.h `fp_grow_sweep_policy`): `grow_sweep` where
    /// candidate k is one `place_policy_quota` of the pending containers on the live table `nodes` (read only, may
    /// be empty; `node_count` None = zeros) followed by `t_max[k]` empty servers of the template standing in domain
    /// `t_domain[k]`, under `strategy`, `preferred_labels`, the spread constraint (`domain`, `t_domain`, `max_skew`;
    /// `t_domain` None or 0 = none), the fallback chain (`relax_mask`, at most `ffi::FP_FALLBACK_MAX_HOPS`; empty =
    /// none) and the quota (`quota` None = none; `quota_used` None = zeros, read only).  No input is changed.
    /// Returns one row of `ffi::FP_GROW_WORDS` and one of `ffi::FP_GROW_POLICY_WORDS` words per candidate and,
    /// with `want_assign`, candidate-major per container: the node in the combined table (`nodes.len() + j` = the
    /// j-th new server, `ffi::FP_NONE` = none), the hop and the reason.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn grow_sweep_policy(&mut self, c: &Containers, reason: Option<&[u8]>, reason_mask: u32, nodes: &Nodes,
                             node_count: Option<&[u32]>, t_cpu: &[u32], t_mem: &[u32], t_labels: &[u32],
                             t_max: Option<&[u32]>, max_new: u32, strategy: u32, preferred_labels: u32,
                             domain: Option<&[u32]>, t_domain: Option<&[u32]>, max_skew: u32, relax_mask: &[u32],
                             quota: Option<&[u32; 3]>, quota_used: Option<&[u32; 3]>, want_assign: bool)
                             -> Result<(Vec<[u32; ffi::FP_GROW_WORDS]>, Vec<[u32; ffi::FP_GROW_POLICY_WORDS]>,
                                        Option<(Vec<u32>, Vec<u8>, Vec<u8>)>), PlanError> {
        let (n, nn, k) = (c.cpu_m.len(), nodes.cpu_free.len(), t_cpu.len());
        if !c.all_len(n) || !nodes.all_len(nn) || t_mem.len() != k || t_labels.len() != k
            || t_max.map_or(false, |m| m.len() != k) || node_count.map_or(false, |x| x.len() != nn)
            || domain.map_or(false, |d| d.len() != nn) || t_domain.map_or(false, |d| d.len() != k)
            || relax_mask.len() > ffi::FP_FALLBACK_MAX_HOPS as usize
            || (reason_mask != 0 && reason.map_or(true, |r| r.len() != n)) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        // the sweep reads the node table only: the mutable pointers of fp_nodes are never written through
        let ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_ptr() as *mut u32,
                                 mem_free: nodes.mem_free.as_ptr() as *mut u32, labels: nodes.labels.as_ptr(),
                                 conflict_used: nodes.conflict_used.as_ptr() as *mut u32,
                                 schedulable: nodes.schedulable.as_ptr() };
        let mut rows = vec![[0u32; ffi::FP_GROW_WORDS]; k];
        let mut prows = vec![[0u32; ffi::FP_GROW_POLICY_WORDS]; k];
        let mut per = if want_assign { Some((vec![ffi::FP_NONE; k * n], vec![0u8; k * n], vec![0u8; k * n])) } else { None };
        let (pa, ph, pr) = per.as_mut().map_or((std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()),
                                               |p| (p.0.as_mut_ptr(), p.1.as_mut_ptr(), p.2.as_mut_ptr()));
        let reason_ptr = if reason_mask != 0 { reason.map_or(std::ptr::null(), |r| r.as_ptr()) } else { std::ptr::null() };
        check(unsafe {
            ffi::fp_grow_sweep_policy(self.ctx, &cs, reason_ptr, reason_mask, &ns,
                                      node_count.map_or(std::ptr::null(), |x| x.as_ptr()), k as u32, t_cpu.as_ptr(),
                                      t_mem.as_ptr(), t_labels.as_ptr(), t_max.map_or(std::ptr::null(), |m| m.as_ptr()),
                                      max_new, strategy, preferred_labels, domain.map_or(std::ptr::null(), |d| d.as_ptr()),
                                      t_domain.map_or(std::ptr::null(), |d| d.as_ptr()), max_skew,
                                      if relax_mask.is_empty() { std::ptr::null() } else { relax_mask.as_ptr() },
                                      relax_mask.len() as u32, quota.map_or(std::ptr::null(), |q| q.as_ptr()),
                                      quota_used.map_or(std::ptr::null(), |q| q.as_ptr()), rows.as_mut_ptr() as *mut u32,
                                      prows.as_mut_ptr() as *mut u32, pa, ph, pr)
        })?;
        Ok((rows, prows, per))
    }

    /// Scored placement (SPEC.md 2.6, fleetplace.h `fp_place_policy`): `strategy` is one of
    /// `ffi::FP_STRATEGY_*`, `preferred_labels` the soft preferred-label mask, `node_count` the
    /// containers already on each node (updated in place; None starts at zero).  `nodes` is
    /// updated in place.  At most `ffi::FP_POLICY_MAX_NODES` nodes (FP_EOVERFLOW).
    pub fn place_policy(&mut self, c: &Containers, nodes: &mut Nodes, level: Option<&[u32]>, strategy: u32,
                        preferred_labels: u32, node_count: Option<&mut [u32]>)
                        -> Result<(Vec<u32>, Vec<u8>), PlanError> {
        let n = c.cpu_m.len();
        let nn = nodes.cpu_free.len();
        if !c.all_len(n) || !nodes.all_len(nn) || level.map_or(false, |l| l.len() != n)
            || node_count.as_ref().map_or(false, |k| k.len() != nn) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                     mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                     conflict_used: nodes.conflict_used.as_mut_ptr(),
                                     schedulable: nodes.schedulable.as_ptr() };
        let (mut assign, mut reason) = (vec![0u32; n], vec![0u8; n]);
        let count_ptr = node_count.map_or(std::ptr::null_mut(), |k| k.as_mut_ptr());
        check(unsafe {
            ffi::fp_place_policy(self.ctx, &cs, &mut ns, level.map_or(std::ptr::null(), |l| l.as_ptr()),
                                 strategy, preferred_labels, count_ptr, assign.as_mut_ptr(), reason.as_mut_ptr())
        })?;
        Ok((assign, reason))
    }

    /// Re-planning a running stage (SPEC.md 2.13, fleetplace.h `fp_replan`): `nodes` is the base table (everything
    /// deducted except these containers' own requests; updated in place) and `prev[c]` the node container c runs
    /// on now (`ffi::FP_NONE` = none).  A container keeps its node while it still fits there -- a cordoned node
    /// keeps what runs on it -- and the others are placed as `place_policy` places them, on the state the seats
    /// left.  Returns (assign, reason, one `ffi::FP_CHANGE_*` value per container, the `ffi::FP_REPLAN_*` words).
    #[allow(clippy::too_many_arguments)]
    pub fn replan(&mut self, c: &Containers, nodes: &mut Nodes, level: Option<&[u32]>, prev: &[u32], strategy: u32,
                  preferred_labels: u32, node_count: Option<&mut [u32]>)
                  -> Result<(Vec<u32>, Vec<u8>, Vec<u8>, [u32; ffi::FP_REPLAN_WORDS]), PlanError> {
        let n = c.cpu_m.len();
        let nn = nodes.cpu_free.len();
        if !c.all_len(n) || !nodes.all_len(nn) || level.map_or(false, |l| l.len() != n) || prev.len() != n
            || node_count.as_ref().map_or(false, |k| k.len() != nn) {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                     mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                     conflict_used: nodes.conflict_used.as_mut_ptr(),
                                     schedulable: nodes.schedulable.as_ptr() };
        let (mut assign, mut reason, mut change) = (vec![0u32; n], vec![0u8; n], vec![0u8; n]);
        let mut summary = [0u32; ffi::FP_REPLAN_WORDS];
        let count_ptr = node_count.map_or(std::ptr::null_mut(), |k| k.as_mut_ptr());
        check(unsafe {
            ffi::fp_replan(self.ctx, &cs, &mut ns, level.map_or(std::ptr::null(), |l| l.as_ptr()), prev.as_ptr(),
                           strategy, preferred_labels, count_ptr, assign.as_mut_ptr(), reason.as_mut_ptr(),
                           change.as_mut_ptr(), summary.as_mut_ptr())
        })?;
        Ok((assign, reason, change, summary))
    }

    /// Scored placement under a hard topology spread (SPEC.md 2.7, fleetplace.h `fp_place_policy_spread`),
    /// the PlacementPolicy's `SpreadConstraint { topology_key, max_skew }`: `domain[n]` is the topology
    /// domain of node n (below `ffi::FP_SPREAD_MAX_DOMAINS`, else FP_EINVAL) and a node is feasible only
    /// while its domain's container count stays within `max_skew` of the emptiest eligible domain.  A
    /// container some node fits but none within the skew has reason `ffi::FP_REASON_SKEW`.
    /// `max_skew = 0` is `place_policy`.
    pub fn place_policy_spread(&mut self, c: &Containers, nodes: &mut Nodes, level: Option<&[u32]>, strategy: u32,
                               preferred_labels: u32, node_count: Option<&mut [u32]>, domain: &[u32], max_skew: u32)
                               -> Result<(Vec<u32>, Vec<u8>), PlanError> {
        let n = c.cpu_m.len();
        let nn = nodes.cpu_free.len();
        if !c.all_len(n) || !nodes.all_len(nn) || level.map_or(false, |l| l.len() != n)
            || node_count.as_ref().map_or(false, |k| k.len() != nn) || domain.len() != nn {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                     mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                     conflict_used: nodes.conflict_used.as_mut_ptr(),
                                     schedulable: nodes.schedulable.as_ptr() };
        let (mut assign, mut reason) = (vec![0u32; n], vec![0u8; n]);
        let count_ptr = node_count.map_or(std::ptr::null_mut(), |k| k.as_mut_ptr());
        check(unsafe {
            ffi::fp_place_policy_spread(self.ctx, &cs, &mut ns, level.map_or(std::ptr::null(), |l| l.as_ptr()),
                                        strategy, preferred_labels, count_ptr, domain.as_ptr(), max_skew,
                                        assign.as_mut_ptr(), reason.as_mut_ptr())
        })?;
        Ok((assign, reason))
    }

    /// Scored placement under a fallback chain (SPEC.md 2.8, fleetplace.h `fp_place_policy_fallback`), the
    /// PlacementPolicy's `FallbackPolicy { relax_order, max_hops }`: `relax_mask[h - 1]` holds the required
    /// label bits hop h gives up (at most `ffi::FP_FALLBACK_MAX_HOPS` hops, else FP_EINVAL).  A container
    /// goes to the feasible node of the smallest (hop, key) and gives a requirement up only when no node of
    /// an earlier hop is feasible.  `spread` is `place_policy_spread`'s `(domain, max_skew)`, None for no
    /// constraint.  Returns (assign, reason, hops): hops[c] is the winner's hop, 0 when rejected.  No masks
    /// is `place_policy_spread`.
    pub fn place_policy_fallback(&mut self, c: &Containers, nodes: &mut Nodes, level: Option<&[u32]>, strategy: u32,
                                 preferred_labels: u32, node_count: Option<&mut [u32]>, spread: Option<(&[u32], u32)>,
                                 relax_mask: &[u32]) -> Result<(Vec<u32>, Vec<u8>, Vec<u8>), PlanError> {
        let n = c.cpu_m.len();
        let nn = nodes.cpu_free.len();
        if !c.all_len(n) || !nodes.all_len(nn) || level.map_or(false, |l| l.len() != n)
            || node_count.as_ref().map_or(false, |k| k.len() != nn) || spread.map_or(false, |(d, _)| d.len() != nn)
            || relax_mask.len() > ffi::FP_FALLBACK_MAX_HOPS as usize {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                     mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                     conflict_used: nodes.conflict_used.as_mut_ptr(),
                                     schedulable: nodes.schedulable.as_ptr() };
        let (mut assign, mut reason, mut hops) = (vec![0u32; n], vec![0u8; n], vec![0u8; n]);
        let count_ptr = node_count.map_or(std::ptr::null_mut(), |k| k.as_mut_ptr());
        let mut masks = [0u32; ffi::FP_FALLBACK_MAX_HOPS as usize];
        masks[..relax_mask.len()].copy_from_slice(relax_mask);
        let (domain, max_skew) = spread.map_or((std::ptr::null(), 0), |(d, k)| (d.as_ptr(), k));
        check(unsafe {
            ffi::fp_place_policy_fallback(self.ctx, &cs, &mut ns, level.map_or(std::ptr::null(), |l| l.as_ptr()),
                                          strategy, preferred_labels, count_ptr, domain, max_skew, masks.as_ptr(),
                                          relax_mask.len() as u32, assign.as_mut_ptr(), reason.as_mut_ptr(),
                                          hops.as_mut_ptr())
        })?;
        Ok((assign, reason, hops))
    }

    /// Scored placement under a resource quota (SPEC.md 2.10, fleetplace.h `fp_place_policy_quota`), the
    /// PlacementPolicy's `ResourceQuota { max_services_per_stage, cpu_cores, memory_gb }` in planner units:
    /// `quota` = [cpu millicores, memory MiB, services], `ffi::FP_QUOTA_UNLIMITED` for no cap in a
    /// dimension; `quota_used` is what the tenant holds already and is updated in place (None starts at
    /// zero).  A container the quota refuses has reason `ffi::FP_REASON_QUOTA` and the mask of the blocking
    /// dimensions (bit `ffi::FP_QUOTA_*`) in the last vector; it is tried on no node and charged nothing.
    /// The other arguments are `place_policy_fallback`'s.  Returns (assign, reason, hops, quota_why).
    /// `max_stages` has no counterpart: it caps the tenant's stage records, not a stage's placement.
    pub fn place_policy_quota(&mut self, c: &Containers, nodes: &mut Nodes, level: Option<&[u32]>, strategy: u32,
                              preferred_labels: u32, node_count: Option<&mut [u32]>, spread: Option<(&[u32], u32)>,
                              relax_mask: &[u32], quota: &[u32; ffi::FP_QUOTA_DIMS],
                              quota_used: Option<&mut [u32; ffi::FP_QUOTA_DIMS]>)
                              -> Result<(Vec<u32>, Vec<u8>, Vec<u8>, Vec<u8>), PlanError> {
        let n = c.cpu_m.len();
        let nn = nodes.cpu_free.len();
        if !c.all_len(n) || !nodes.all_len(nn) || level.map_or(false, |l| l.len() != n)
            || node_count.as_ref().map_or(false, |k| k.len() != nn) || spread.map_or(false, |(d, _)| d.len() != nn)
            || relax_mask.len() > ffi::FP_FALLBACK_MAX_HOPS as usize {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let cs = ffi::fp_containers { n: n as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                      req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
        let mut ns = ffi::fp_nodes { n: nn as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                     mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                     conflict_used: nodes.conflict_used.as_mut_ptr(),
                                     schedulable: nodes.schedulable.as_ptr() };
        let (mut assign, mut reason, mut hops, mut why) = (vec![0u32; n], vec![0u8; n], vec![0u8; n], vec![0u8; n]);
        let count_ptr = node_count.map_or(std::ptr::null_mut(), |k| k.as_mut_ptr());
        let used_ptr = quota_used.map_or(std::ptr::null_mut(), |u| u.as_mut_ptr());
        let mut masks = [0u32; ffi::FP_FALLBACK_MAX_HOPS as usize];
        masks[..relax_mask.len()].copy_from_slice(relax_mask);
        let (domain, max_skew) = spread.map_or((std::ptr::null(), 0), |(d, k)| (d.as_ptr(), k));
        check(unsafe {
            ffi::fp_place_policy_quota(self.ctx, &cs, &mut ns, level.map_or(std::ptr::null(), |l| l.as_ptr()),
                                       strategy, preferred_labels, count_ptr, domain, max_skew, masks.as_ptr(),
                                       relax_mask.len() as u32, assign.as_mut_ptr(), reason.as_mut_ptr(),
                                       hops.as_mut_ptr(), quota.as_ptr(), used_ptr, why.as_mut_ptr())
        })?;
        Ok((assign, reason, hops, why))
    }

    /// One stage's whole dry-run plan in one call (fleetplace.h `fp_plan_stage`, the
    /// `fleet up --dry-run` path of up.rs:57-136): the legacy order, the Kahn levels and start
    /// order and, with `placement = Some((containers, nodes))` (container v = vertex v), the
    /// stage-2 first feasible server and count per service and the FFD plan, `nodes` updated
    /// in place.  A stage of <= 512 services is one kernel launch.
    pub fn plan_stage(&mut self, row_ptr: &[u32], col: &[u32], has_deps: &[u8],
                      placement: Option<(&Containers, &mut Nodes)>) -> Result<StagePlan, PlanError> {
        let v = has_deps.len();
        if v > 0 && row_ptr.len() != v + 1 {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        let g = ffi::fp_graph { n_vertices: v as u32, n_edges: col.len() as u32, row_ptr: row_ptr.as_ptr(),
                                col: if col.is_empty() { std::ptr::null() } else { col.as_ptr() },
                                has_deps: has_deps.as_ptr() };
        let mut out = StagePlan { perm: vec![0; v], level: vec![0; v], order: vec![0; v], n_cycle: 0,
                                  first: vec![], count: vec![], assign: vec![], reason: vec![] };
        let rc = match placement {
            None => unsafe {
                ffi::fp_plan_stage(self.ctx, &g, std::ptr::null(), std::ptr::null_mut(), out.perm.as_mut_ptr(),
                                   out.level.as_mut_ptr(), out.order.as_mut_ptr(), &mut out.n_cycle,
                                   std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(),
                                   std::ptr::null_mut())
            },
            Some((c, nodes)) => {
                if !c.all_len(v) || !nodes.all_len(nodes.cpu_free.len()) {
                    return Err(PlanError(ffi::FP_EINVAL));
                }
                let cs = ffi::fp_containers { n: v as u32, cpu_m: c.cpu_m.as_ptr(), mem_mib: c.mem_mib.as_ptr(),
                                              req_labels: c.req_labels.as_ptr(), conflict: c.conflict.as_ptr() };
                let mut ns = ffi::fp_nodes { n: nodes.cpu_free.len() as u32, cpu_free: nodes.cpu_free.as_mut_ptr(),
                                             mem_free: nodes.mem_free.as_mut_ptr(), labels: nodes.labels.as_ptr(),
                                             conflict_used: nodes.conflict_used.as_mut_ptr(),
                                             schedulable: nodes.schedulable.as_ptr() };
                out.first = vec![0; v];
                out.count = vec![0; v];
                out.assign = vec![0; v];
                out.reason = vec![0; v];
                unsafe {
                    ffi::fp_plan_stage(self.ctx, &g, &cs, &mut ns, out.perm.as_mut_ptr(), out.level.as_mut_ptr(),
                                       out.order.as_mut_ptr(), &mut out.n_cycle, out.first.as_mut_ptr(),
                                       out.count.as_mut_ptr(), out.assign.as_mut_ptr(), out.reason.as_mut_ptr())
                }
            }
        };
        check(rc)?;
        Ok(out)
    }
}

/// The result of [`Planner::plan_stage`], per vertex of the stage graph.  The placement
/// vectors are empty for a stage planned without servers.
pub struct StagePlan {
    /// A1 legacy start order (engine.rs:64-85)
    pub perm: Vec<u32>,
    /// A2 start level (FP_NONE = CYCLE) and the (level, index) start order
    pub level: Vec<u32>,
    pub order: Vec<u32>,
    pub n_cycle: u32,
    /// stage 2 on the pristine server table: first feasible server (FP_NONE) and count
    pub first: Vec<u32>,
    pub count: Vec<u32>,
    /// A6 FFD: server per service (FP_NONE if unplaced) and reason (FP_REASON_*)
    pub assign: Vec<u32>,
    pub reason: Vec<u8>,
}

impl Planner {
    /// What-if planning over `b.n_scen` independent scenarios (fleetplace.h `fp_place_batch`):
    /// every scenario's plan, its packed cost `(n_rejected:24 | n_nodes_used:24 | id:16)` and
    /// the updated node tables, in `b` (scenario-major arrays).
    pub fn place_batch(&mut self, b: &mut Batch) -> Result<(), PlanError> {
        let (s, c, n) = (b.n_scen as usize, b.n_containers as usize, b.n_nodes as usize);
        // every array fp_place_batch reads or writes must hold S * C (containers) or S * N (nodes)
        let ok = b.containers.all_len(s * c) && b.nodes.all_len(s * n)
            && b.level.as_ref().map_or(true, |l| l.len() == s * c);
        if !ok {
            return Err(PlanError(ffi::FP_EINVAL));
        }
        b.assign.resize(s * c, 0);
        b.reason.resize(s * c, 0);
        b.cost.resize(s, 0);
        let fb = ffi::fp_batch {
            n_scen: b.n_scen, scen_base: b.scen_base, n_containers: b.n_containers, n_nodes: b.n_nodes,
            cpu_m: b.containers.cpu_m.as_ptr(), mem_mib: b.containers.mem_mib.as_ptr(),
            req_labels: b.containers.req_labels.as_ptr(), conflict: b.containers.conflict.as_ptr(),
            level: b.level.as_ref().map_or(std::ptr::null(), |l| l.as_ptr()),
            cpu_free: b.nodes.cpu_free.as_mut_ptr(), mem_free: b.nodes.mem_free.as_mut_ptr(),
            labels: b.nodes.labels.as_ptr(), conflict_used: b.nodes.conflict_used.as_mut_ptr(),
            schedulable: b.nodes.schedulable.as_ptr(), assign: b.assign.as_mut_ptr(), reason: b.reason.as_mut_ptr(),
            cost: b.cost.as_mut_ptr(),
        };
        check(unsafe { ffi::fp_place_batch(self.ctx, &fb) })
    }

    /// The same planning on HBM-resident arrays (fleetplace.h `fp_dev_place_batch`, asynchronous
    /// on the context's stream), then the best scenario on the device
    /// (`fp_dev_argmin_cost` into `best_dev`).  Kernel errors surface at [`Planner::sync`].
    ///
    /// # Safety
    /// Every pointer in `b` and `best_dev` must be device memory of this context's GPU, sized as
    /// fleetplace.h documents, and stay valid until the stream has drained.
    pub unsafe fn dev_place_batch(&mut self, b: &ffi::fp_batch, best_dev: *mut u32) -> Result<(), PlanError> {
        check(ffi::fp_dev_place_batch(self.ctx, b))?;
        if !b.cost.is_null() && !best_dev.is_null() && b.n_scen > 0 {
            check(ffi::fp_dev_argmin_cost(self.ctx, b.cost, b.n_scen, best_dev))?;
        }
        Ok(())
    }

    /// Waits for the context's asynchronous calls and reports their first kernel error.
    pub fn sync(&mut self) -> Result<(), PlanError> {
        check(unsafe { ffi::fp_ctx_sync(self.ctx) })
    }

    /// Device workspace a batch of this shape takes (grown once per context, then reused).
    pub fn workspace_bytes(&mut self, n_scen: u32, n_containers: u32, n_nodes: u32) -> Result<u64, PlanError> {
        let mut bytes = 0u64;
        check(unsafe { ffi::fp_place_ws_bytes(self.ctx, n_scen, n_containers, n_nodes, &mut bytes) })?;
        Ok(bytes)
    }

    /// The placement pipeline a batch of this shape runs (`FP_GEOM_*` indices).
    pub fn geometry(&mut self, n_scen: u32, n_containers: u32, n_nodes: u32)
                    -> Result<[u32; ffi::FP_GEOM_COUNT], PlanError> {
        let mut out = [0u32; ffi::FP_GEOM_COUNT];
        check(unsafe { ffi::fp_place_geometry(self.ctx, n_scen, n_containers, n_nodes, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// A per-context option (`FP_OPT_*`; `FP_OPT_AUTO` restores the default).
    pub fn set_option(&mut self, option: i32, value: i64) -> Result<(), PlanError> {
        check(unsafe { ffi::fp_ctx_set_option(self.ctx, option, value) })
    }
}

impl Drop for Planner {
    fn drop(&mut self) {
        unsafe { ffi::fp_ctx_destroy(self.ctx) }
    }
}

/// Container requests (SoA): millicores, MiB, required label bits, conflict bits
/// (host-port bits 0-15 | anti-affinity group bits 16-31).
pub struct Containers {
    pub cpu_m: Vec<u32>,
    pub mem_mib: Vec<u32>,
    pub req_labels: Vec<u32>,
    pub conflict: Vec<u32>,
}

impl Containers {
    /// every array holds exactly `n` elements
    fn all_len(&self, n: usize) -> bool {
        self.cpu_m.len() == n && self.mem_mib.len() == n && self.req_labels.len() == n && self.conflict.len() == n
    }
}

/// Node table (SoA) in node-index order (`stage.servers` order, or `ORDER BY slug` for
/// the controlplane registry, db.rs:741-750).
pub struct Nodes {
    pub cpu_free: Vec<u32>,
    pub mem_free: Vec<u32>,
    pub labels: Vec<u32>,
    pub conflict_used: Vec<u32>,
    pub schedulable: Vec<u8>,
}

impl Nodes {
    /// every array holds exactly `n` elements
    fn all_len(&self, n: usize) -> bool {
        self.cpu_free.len() == n && self.mem_free.len() == n && self.labels.len() == n
            && self.conflict_used.len() == n && self.schedulable.len() == n
    }
}

/// `n_scen` independent what-if scenarios of `n_containers` x `n_nodes`, scenario-major
/// (`containers.*[s * C + i]`, `nodes.*[s * N + j]`); outputs filled by [`Planner::place_batch`].
pub struct Batch {
    pub n_scen: u32,
    /// global id of scenario 0 in the packed costs (scen_base + n_scen <= 65536)
    pub scen_base: u32,
    pub n_containers: u32,
    pub n_nodes: u32,
    pub containers: Containers,
    pub nodes: Nodes,
    /// start levels ([S * C]); `FP_NONE` marks a CYCLE member, which is not placed
    pub level: Option<Vec<u32>>,
    pub assign: Vec<u32>,
    pub reason: Vec<u8>,
    pub cost: Vec<u64>,
}

/// The outcome of [`plan_scenarios`]: every scenario's packed cost, the best scenario (lowest
/// cost; the id field breaks ties towards the lowest id) and its plan.
pub struct ScenarioPlans {
    pub cost: Vec<u64>,
    pub best: u32,
    pub assign: Vec<u32>,
    pub reason: Vec<u8>,
}

/// Unpacks a packed scenario cost: (rejected containers, nodes used, scenario id).
pub fn unpack_cost(c: u64) -> (u32, u32, u32) {
    ((c >> 40) as u32, ((c >> 16) & 0xFF_FFFF) as u32, (c & 0xFFFF) as u32)
}

/// Plans every scenario of `b` on this thread's GPU and picks the best one (the what-if
/// surface of the controlplane: one target per deploy, deploy.rs:441-451).
pub fn plan_scenarios(b: &mut Batch) -> Result<ScenarioPlans, PlanError> {
    with_planner(|p| p.place_batch(b))?;
    let c = b.n_containers as usize;
    let best = b.cost.iter().enumerate().min_by_key(|&(i, &v)| (v, i)).map_or(0, |(i, _)| i);
    Ok(ScenarioPlans { cost: b.cost.clone(), best: best as u32, assign: b.assign[best * c..(best + 1) * c].to_vec(),
                       reason: b.reason[best * c..(best + 1) * c].to_vec() })
}

thread_local! {
    static PLANNER: RefCell<Option<Planner>> = const { RefCell::new(None) };
}

/// Runs `f` with this thread's planner on device 0 (created on first use).
pub fn with_planner<R>(f: impl FnOnce(&mut Planner) -> Result<R, PlanError>) -> Result<R, PlanError> {
    PLANNER.with(|p| {
        let mut p = p.borrow_mut();
        if p.is_none() {
            *p = Some(Planner::new(0)?);
        }
        f(p.as_mut().unwrap())
    })
}

/// engine.rs:71-80 predicate per position: known in `flow.services` AND depends_on non-empty.
fn has_deps_vector(services: &[String], flow: &Flow) -> Vec<u8> {
    services.iter().map(|n| flow.services.get(n).map_or(0, |s| (!s.depends_on.is_empty()) as u8)).collect()
}

/// Same signature and output as `fleetflow_container::order_by_dependencies`
/// (crates/fleetflow-container/src/engine.rs:64-85), computed by the GPU planner.
/// Panics when no MI355X is available (the reference function is infallible; use
/// [`try_order_by_dependencies`] to handle the error).
pub fn order_by_dependencies(services: &[String], flow: &Flow) -> Vec<String> {
    try_order_by_dependencies(services, flow).expect("fleetflow-placement: GPU planner unavailable")
}

pub fn try_order_by_dependencies(services: &[String], flow: &Flow) -> Result<Vec<String>, PlanError> {
    if services.is_empty() {
        return Ok(Vec::new());
    }
    let perm = with_planner(|p| p.legacy_order(&has_deps_vector(services, flow)))?;
    Ok(perm.iter().map(|&i| services[i as usize].clone()).collect())
}

/// Reversed CSR of a stage's `depends_on` graph (SPEC.md 1): vertex = first occurrence of a
/// name in stage order; deps outside the stage add no edge; duplicate deps give duplicate
/// edges.  Returns (vertex of each position, row_ptr, col, has_deps per vertex).
pub fn stage_graph(services: &[String], flow: &Flow) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<u8>) {
    let mut vid: HashMap<&str, u32> = HashMap::new();
    let mut names: Vec<&str> = Vec::new();
    let pos: Vec<u32> = services.iter().map(|n| *vid.entry(n.as_str()).or_insert_with(|| {
        names.push(n.as_str());
        (names.len() - 1) as u32
    })).collect();
    let v = names.len();
    let mut has_deps = vec![0u8; v];
    let mut edges: Vec<(u32, u32)> = Vec::new();
    for (i, n) in names.iter().enumerate() {
        if let Some(svc) = flow.services.get(*n) {
            if !svc.depends_on.is_empty() {
                has_deps[i] = 1;
                for d in &svc.depends_on {
                    if let Some(&dv) = vid.get(d.as_str()) {
                        edges.push((dv, i as u32));
                    }
                }
            }
        }
    }
    let mut row_ptr = vec![0u32; v + 1];
    for &(d, _) in &edges {
        row_ptr[d as usize + 1] += 1;
    }
    for i in 0..v {
        row_ptr[i + 1] += row_ptr[i];
    }
    let mut fill = row_ptr[..v].to_vec();
    let mut col = vec![0u32; edges.len()];
    for &(d, t) in &edges {
        col[fill[d as usize] as usize] = t;
        fill[d as usize] += 1;
    }
    (pos, row_ptr, col, has_deps)
}

/// Kahn start level of every position of `services` (`None` = CYCLE: the reference's
/// never-constructed `FlowError::CircularDependency`, crates/fleetflow-core/src/error.rs:42-43).
pub fn start_levels(services: &[String], flow: &Flow) -> Result<Vec<Option<u32>>, PlanError> {
    if services.is_empty() {
        return Ok(Vec::new());
    }
    let (pos, row_ptr, col, has_deps) = stage_graph(services, flow);
    let (level, _, _) = with_planner(|p| p.levelize(&row_ptr, &col, &has_deps))?;
    Ok(pos.iter().map(|&v| match level[v as usize] { ffi::FP_NONE => None, l => Some(l) }).collect())
}

/// Parallel start waves for `DeployEngine::create_and_start` (engine.rs:355-452): wave k holds
/// the services at level k, in declaration order; every in-stage dependency of a wave-k
/// service is in an earlier wave.  CYCLE services are in no wave (returned separately).
pub fn start_waves(services: &[String], flow: &Flow) -> Result<(Vec<Vec<String>>, Vec<String>), PlanError> {
    let levels = start_levels(services, flow)?;
    let mut by_level: std::collections::BTreeMap<u32, Vec<String>> = Default::default();
    let mut cycle = Vec::new();
    let mut seen = std::collections::HashSet::new();
    for (name, lv) in services.iter().zip(levels) {
        if !seen.insert(name.as_str()) {
            continue;
        }
        match lv {
            Some(l) => by_level.entry(l).or_default().push(name.clone()),
            None => cycle.push(name.clone()),
        }
    }
    Ok((by_level.into_values().collect(), cycle))
}

/// crates/fleetflow-controlplane/src/handlers/deploy.rs:390-394, as the reference computes it:
/// `flow.stages.get(stage).and_then(|s| s.servers.first().cloned())`.  `None` means the caller's
/// "local" fallback (:396-398).  Pure Rust: choosing the first declared server needs no planner
/// (and so no GPU); [`place_stage`] is the capacity-aware fan-out that replaces it.
pub fn resolve_target_server(flow: &Flow, stage_name: &str) -> Option<String> {
    flow.stages.get(stage_name).and_then(|s| s.servers.first().cloned())
}

/// Per-service server choice for a stage (the fan-out deploy.rs:388-389 leaves for later):
/// first-fit-decreasing of the stage's services (requests in `c`, stage order) over its servers
/// (`nodes`, `stage.servers` order), on the GPU.  Returns the server of every service, `None`
/// for one that fits nowhere (NOFIT).  With unconstrained capacity every service lands on the
/// first server, i.e. [`resolve_target_server`].
pub fn place_stage(flow: &Flow, stage_name: &str, c: &Containers, nodes: &mut Nodes)
                   -> Result<Vec<Option<String>>, PlanError> {
    let Some(stage) = flow.stages.get(stage_name) else { return Err(PlanError(ffi::FP_EINVAL)) };
    if nodes.cpu_free.len() != stage.servers.len() || c.cpu_m.len() != stage.services.len() {
        return Err(PlanError(ffi::FP_EINVAL));
    }
    let (assign, _) = with_planner(|p| p.place(c, nodes, None))?;
    Ok(assign.iter().map(|&a| if a == ffi::FP_NONE { None } else { Some(stage.servers[a as usize].clone()) }).collect())
}

/// Why the services [`place_stage`] could not place have no server (SPEC.md 2.9): `assign` is its result and
/// `nodes` the table it left.  Returns, for every unplaced service in stage order, its position in the
/// stage and its row of `ffi::FP_EXPLAIN_WORDS` words (`ffi::FP_EXPLAIN_*`: per-cause server counts, the
/// causes that fail on every server, the missing labels, the nearest server).
pub fn explain_stage(flow: &Flow, stage_name: &str, c: &Containers, nodes: &Nodes, assign: &[Option<String>])
                     -> Result<Vec<(usize, [u32; ffi::FP_EXPLAIN_WORDS])>, PlanError> {
    let Some(stage) = flow.stages.get(stage_name) else { return Err(PlanError(ffi::FP_EINVAL)) };
    if nodes.cpu_free.len() != stage.servers.len() || c.cpu_m.len() != stage.services.len()
        || assign.len() != stage.services.len() {
        return Err(PlanError(ffi::FP_EINVAL));
    }
    let sel: Vec<u32> = assign.iter().enumerate().filter(|(_, a)| a.is_none()).map(|(i, _)| i as u32).collect();
    if sel.is_empty() {
        return Ok(Vec::new());
    }
    let rows = with_planner(|p| p.explain(c, nodes, Some(&sel), 0))?;
    Ok(sel.iter().map(|&i| i as usize).zip(rows).collect())
}

/// "Can this server be taken out?" for every server of a stage (SPEC.md 2.11; the `drain` scheduling state of
/// crates/fleetflow-controlplane/src/model.rs:435-442): `assign` is the running plan ([`place_stage`]'s result)
/// and `nodes` the live table it left.  Each server is drained on its own, from the same live state.  Returns,
/// per server in `stage.servers` order, its slug, the moves `(service, new server)` of the services it runs
/// (`None` = stranded, in stage order) and its row of `ffi::FP_DRAIN_WORDS` words (`ffi::FP_DRAIN_*`).
#[allow(clippy::type_complexity)]
pub fn drain_sweep(flow: &Flow, stage_name: &str, c: &Containers, nodes: &Nodes, assign: &[Option<String>],
                   strategy: u32, preferred_labels: u32, node_count: Option<&[u32]>)
                   -> Result<Vec<(String, Vec<(String, Option<String>)>, [u32; ffi::FP_DRAIN_WORDS])>, PlanError> {
    let Some(stage) = flow.stages.get(stage_name) else { return Err(PlanError(ffi::FP_EINVAL)) };
    if nodes.cpu_free.len() != stage.servers.len() || c.cpu_m.len() != stage.services.len()
        || assign.len() != stage.services.len() {
        return Err(PlanError(ffi::FP_EINVAL));
    }
    let mut running = Vec::with_capacity(assign.len());
    for a in assign {
        running.push(match a {
            None => ffi::FP_NONE,
            Some(slug) => match stage.servers.iter().position(|s| s == slug) {
                Some(n) => n as u32,
                None => return Err(PlanError(ffi::FP_EINVAL)),
            },
        });
    }
    let group: Vec<u32> = (0..stage.servers.len() as u32).collect();
    let (out, _, rows) = with_planner(|p| {
        p.drain_sweep(c, nodes, &running, &group, group.len() as u32, strategy, preferred_labels, node_count)
    })?;
    Ok(stage.servers.iter().enumerate().map(|(k, slug)| {
        let moves = running.iter().enumerate().filter(|(_, &n)| n == k as u32).map(|(v, _)| {
            let to = if out[v] == ffi::FP_NONE { None } else { Some(stage.servers[out[v] as usize].clone()) };
            (stage.services[v].clone(), to)
        }).collect();
        (slug.clone(), moves, rows[k])
    }).collect())
}

/// `fp_strategy` of a tenant `PlacementPolicy.strategy` string
/// (crates/fleetflow-controlplane/src/model.rs:56-95); None for anything else.
pub fn strategy_from_policy(strategy: &str) -> Option<u32> {
    match strategy {
        "spread_across_pool" => Some(ffi::FP_STRATEGY_SPREAD),
        "pack_into_dedicated" => Some(ffi::FP_STRATEGY_PACK),
        "fill_lowest" => Some(ffi::FP_STRATEGY_FILL_LOWEST),
        _ => None,
    }
}

/// `place_stage` under a placement strategy (SPEC.md 2.6): the same tables, the server chosen by the
/// strategy's key among the feasible ones instead of the first.  `preferred_labels` is the soft
/// preferred-label mask in the stage's label dictionary; `node_count` the containers already on each
/// server (None = none).
pub fn place_stage_with_policy(flow: &Flow, stage_name: &str, c: &Containers, nodes: &mut Nodes, strategy: u32,
                               preferred_labels: u32, node_count: Option<&mut [u32]>)
                               -> Result<Vec<Option<String>>, PlanError> {
    let Some(stage) = flow.stages.get(stage_name) else { return Err(PlanError(ffi::FP_EINVAL)) };
    if nodes.cpu_free.len() != stage.servers.len() || c.cpu_m.len() != stage.services.len() {
        return Err(PlanError(ffi::FP_EINVAL));
    }
    let (assign, _) = with_planner(|p| p.place_policy(c, nodes, None, strategy, preferred_labels, node_count))?;
    Ok(assign.iter().map(|&a| if a == ffi::FP_NONE { None } else { Some(stage.servers[a as usize].clone()) }).collect())
}

/// `place_stage_with_policy` under the tenant's resource quota (SPEC.md 2.10): `quota` and `quota_used` as
/// in [`Planner::place_policy_quota`].  Per service: its server, or None with the reason
/// (`ffi::FP_REASON_QUOTA` for a service the quota refused) and the mask of the blocking dimensions.
pub fn place_stage_with_quota(flow: &Flow, stage_name: &str, c: &Containers, nodes: &mut Nodes, strategy: u32,
                              preferred_labels: u32, node_count: Option<&mut [u32]>,
                              quota: &[u32; ffi::FP_QUOTA_DIMS], quota_used: Option<&mut [u32; ffi::FP_QUOTA_DIMS]>)
                              -> Result<Vec<(Option<String>, u8, u8)>, PlanError> {
    let Some(stage) = flow.stages.get(stage_name) else { return Err(PlanError(ffi::FP_EINVAL)) };
    if nodes.cpu_free.len() != stage.servers.len() || c.cpu_m.len() != stage.services.len() {
        return Err(PlanError(ffi::FP_EINVAL));
    }
    let (assign, reason, _, why) = with_planner(|p| {
        p.place_policy_quota(c, nodes, None, strategy, preferred_labels, node_count, None, &[], quota, quota_used)
    })?;
    Ok(assign.iter().zip(reason.iter().zip(why.iter()))
        .map(|(&a, (&r, &w))| (if a == ffi::FP_NONE { None } else { Some(stage.servers[a as usize].clone()) }, r, w))
        .collect())
}

/// What `fleet up --dry-run` prints for a stage (up.rs:57-136), planned in one call: the
/// reference's start order, the start level of every service (`None` = CYCLE) and, when the
/// stage has servers and `placement` carries their tables, each service's server.  A stage
/// whose service list repeats a name is planned per vertex (first occurrence) and mapped back.
pub fn dry_run_stage(services: &[String], flow: &Flow, placement: Option<(&Containers, &mut Nodes)>)
                     -> Result<(Vec<String>, Vec<Option<u32>>, Option<Vec<Option<u32>>>), PlanError> {
    if services.is_empty() {
        return Ok((Vec::new(), Vec::new(), placement.map(|_| Vec::new())));
    }
    let (pos, row_ptr, col, has_deps) = stage_graph(services, flow);
    let placed = placement.is_some();
    let plan = with_planner(|p| p.plan_stage(&row_ptr, &col, &has_deps, placement))?;
    // the legacy order runs over positions (engine.rs:64-85 keeps duplicates); without
    // duplicates positions and vertices coincide
    let order = if pos.len() == has_deps.len() {
        plan.perm.iter().map(|&i| services[i as usize].clone()).collect()
    } else {
        try_order_by_dependencies(services, flow)?
    };
    let levels = pos.iter().map(|&v| match plan.level[v as usize] { ffi::FP_NONE => None, l => Some(l) }).collect();
    let servers = placed.then(|| pos.iter().map(|&v| match plan.assign[v as usize] {
        ffi::FP_NONE => None,
        a => Some(a),
    }).collect());
    Ok((order, levels, servers))
}

#[cfg(all(test, feature = "gpu-tests"))]
mod tests {
    //! The reference's own known answers (engine.rs:603-666), on the GPU.
    use super::*;
    use fleetflow_core::{Flow, Service};

    fn flow(deps: &[(&str, &[&str])]) -> Flow {
        let mut f = Flow { name: "t".into(), services: Default::default(), stages: Default::default(),
                           providers: Default::default(), servers: Default::default(), registry: None,
                           variables: Default::default(), tenant: None };
        for (n, d) in deps {
            let mut s = Service::default();
            s.depends_on = d.iter().map(|x| x.to_string()).collect();
            f.services.insert(n.to_string(), s);
        }
        f
    }
    fn names(v: &[&str]) -> Vec<String> { v.iter().map(|s| s.to_string()).collect() }

    #[test]
    fn order_no_deps() {
        let f = flow(&[("web", &[]), ("db", &[])]);
        assert_eq!(order_by_dependencies(&names(&["web", "db"]), &f), names(&["web", "db"]));
    }

    #[test]
    fn order_with_deps() {
        let f = flow(&[("web", &["db"]), ("db", &[])]);
        assert_eq!(order_by_dependencies(&names(&["web", "db"]), &f), names(&["db", "web"]));
    }

    #[test]
    fn order_mixed() {
        let f = flow(&[("api", &["db"]), ("db", &[]), ("redis", &[]), ("worker", &["redis", "db"])]);
        let out = order_by_dependencies(&names(&["api", "db", "redis", "worker"]), &f);
        assert_eq!(out, names(&["db", "redis", "api", "worker"]));
    }

    #[test]
    fn scenarios_pick_the_cheapest_plan() {
        // two scenarios of two containers on one node: scenario 1's node is too small for
        // one of them, so scenario 0 (nothing rejected) is the best plan
        let c = Containers { cpu_m: vec![500, 500, 500, 500], mem_mib: vec![64; 4], req_labels: vec![0; 4],
                             conflict: vec![0; 4] };
        let nodes = Nodes { cpu_free: vec![1000, 600], mem_free: vec![1024, 1024], labels: vec![0; 2],
                            conflict_used: vec![0; 2], schedulable: vec![1; 2] };
        let mut b = Batch { n_scen: 2, scen_base: 0, n_containers: 2, n_nodes: 1, containers: c, nodes, level: None,
                            assign: vec![], reason: vec![], cost: vec![] };
        let p = plan_scenarios(&mut b).unwrap();
        assert_eq!(p.best, 0);
        assert_eq!(unpack_cost(p.cost[1]), (1, 1, 1));
        assert_eq!(p.assign, vec![0, 0]);
    }

    #[test]
    fn waves_cross_every_edge() {
        let f = flow(&[("c", &["b"]), ("b", &["a"]), ("a", &[])]);
        let (waves, cycle) = start_waves(&names(&["c", "b", "a"]), &f).unwrap();
        assert_eq!(waves, vec![names(&["a"]), names(&["b"]), names(&["c"])]);
        assert!(cycle.is_empty());
    }
}
