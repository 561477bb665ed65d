// fp_rows.h -- the staged buffers of the host-pointer entry points as fp_row lists (fp_layout.h): one row per
// device buffer, in the order of the takes.  fp_ctx.hip sizes the staging arena from these lists, copies in and
// copies back by them; nothing else says how many bytes a call stages.  Free of HIP like fp_layout.h, so that
// the CPU test walks the same lists the library does.
#pragma once
#include <stdint.h>
#include "../../include/fleetplace.h"
#include "fp_layout.h"

// scored placement (fp_policy.hip, SPEC.md 2.6 to 2.10): what a call has besides its batch.  Not ABI: the
// exports of fp_ctx.hip fill in the fields their signature has.  Only strategy [S] is required.
struct fp_policy_opts {
    const uint32_t *strategy = nullptr, *preferred = nullptr;  // [S] each
    uint32_t *node_count = nullptr;                            // [S][N], in/out
    // topology spread (2.7): domain [S][N], max_skew [S]; either one null = no constraint
    const uint32_t *domain = nullptr, *max_skew = nullptr;
    // fallback chain (2.8): relax_mask [S][4], n_hops [S]; either one null = no fallback.  hops [S][C]
    // receives the winner's hop: all zero when the call has no chain
    const uint32_t *relax_mask = nullptr, *n_hops = nullptr;
    uint8_t *hops = nullptr;
    // resource quota (2.10): quota [S][3], null = no quota; quota_used [S][3] (in/out) and quota_why
    // [S][C] are untouched without quota
    const uint32_t *quota = nullptr;
    uint32_t *quota_used = nullptr;
    uint8_t *quota_why = nullptr;
};

template <class H, class D>
static inline fp_row fp_row_in(const H *h, size_t n, D **d) {  // an input; null = absent
    return {h, nullptr, n * sizeof(H), (void **)d, false};
}
template <class H, class D>
static inline fp_row fp_row_io(H *h, size_t n, D **d) {  // an input that comes back; null = absent
    return {h, h, n * sizeof(H), (void **)d, false};
}
template <class H>
static inline fp_row fp_row_out(H *h, size_t n, H **d) {  // a result the kernels always write; null = not copied back
    return {nullptr, h, n * sizeof(H), (void **)d, true};
}
template <class H>
static inline fp_row fp_row_opt(H *h, size_t n, H **d) {  // a result written only when the caller asks for it
    return {nullptr, h, n * sizeof(H), (void **)d, h != nullptr};
}
constexpr int FP_MAX_ROWS = 32;

// A host batch `b` as device batch `d`: its ten input arrays, then (scored placement: `o` and `dopt` non-null)
// the policy inputs, then assign / reason / cost and the policy outputs the caller asked for.  The node state,
// node_count and quota_used come back.  Returns the number of rows.
static inline int fp_batch_rows(const fp_batch *b, const fp_policy_opts *o, fp_batch *d, fp_policy_opts *dopt,
                                fp_row *r) {
    const size_t S = b->n_scen, SC = S * b->n_containers, SN = S * b->n_nodes;
    *d = *b;
    int n = 0;
    r[n++] = fp_row_in(b->cpu_m, SC, &d->cpu_m);
    r[n++] = fp_row_in(b->mem_mib, SC, &d->mem_mib);
    r[n++] = fp_row_in(b->req_labels, SC, &d->req_labels);
    r[n++] = fp_row_in(b->conflict, SC, &d->conflict);
    r[n++] = fp_row_in(b->level, SC, &d->level);
    r[n++] = fp_row_io(b->cpu_free, SN, &d->cpu_free);
    r[n++] = fp_row_io(b->mem_free, SN, &d->mem_free);
    r[n++] = fp_row_in(b->labels, SN, &d->labels);
    r[n++] = fp_row_io(b->conflict_used, SN, &d->conflict_used);
    r[n++] = fp_row_in(b->schedulable, SN, &d->schedulable);
    if (o) {
        r[n++] = fp_row_in(o->strategy, S, &dopt->strategy);
        r[n++] = fp_row_in(o->preferred, S, &dopt->preferred);
        r[n++] = fp_row_io(o->node_count, SN, &dopt->node_count);
        r[n++] = fp_row_in(o->domain, SN, &dopt->domain);
        r[n++] = fp_row_in(o->max_skew, S, &dopt->max_skew);
        r[n++] = fp_row_in(o->relax_mask, S * FP_FALLBACK_MAX_HOPS, &dopt->relax_mask);
        r[n++] = fp_row_in(o->n_hops, S, &dopt->n_hops);
        r[n++] = fp_row_in(o->quota, S * FP_QUOTA_DIMS, &dopt->quota);
        r[n++] = fp_row_io(o->quota_used, S * FP_QUOTA_DIMS, &dopt->quota_used);
    }
    r[n++] = fp_row_out(b->assign, SC, &d->assign);
    r[n++] = fp_row_out(b->reason, SC, &d->reason);
    r[n++] = fp_row_out(b->cost, S, &d->cost);
    if (o) {
        r[n++] = fp_row_opt(o->hops, SC, &dopt->hops);
        r[n++] = fp_row_opt(o->quota_why, SC, &dopt->quota_why);
    }
    return n;
}

// fp_replan / fp_replan_batch (SPEC.md 2.13): the rows of a scored batch (`o` holds strategy, preferred and
// node_count), then prev, then the two results the caller may ask for
struct fp_replan_dev {
    const uint32_t *prev;
    uint8_t *change;
    uint32_t *summary;
};
static inline int fp_replan_rows(const fp_batch *b, const fp_policy_opts *o, const uint32_t *prev, uint8_t *change_out,
                                 uint32_t *summary_out, fp_batch *d, fp_policy_opts *dopt, fp_replan_dev *dr,
                                 fp_row *r) {
    const size_t S = b->n_scen, SC = S * b->n_containers;
    int n = fp_batch_rows(b, o, d, dopt, r);
    r[n++] = fp_row_in(prev, SC, &dr->prev);
    r[n++] = fp_row_opt(change_out, SC, &dr->change);
    r[n++] = fp_row_opt(summary_out, S * FP_REPLAN_WORDS, &dr->summary);
    return n;
}

// one scenario's container table as inputs (four rows, in this order)
static inline int fp_cont_rows(const fp_containers *cs, fp_containers *dc, fp_row *r) {
    const size_t C = cs->n;
    *dc = *cs;
    int n = 0;
    r[n++] = fp_row_in(cs->cpu_m, C, &dc->cpu_m);
    r[n++] = fp_row_in(cs->mem_mib, C, &dc->mem_mib);
    r[n++] = fp_row_in(cs->req_labels, C, &dc->req_labels);
    r[n++] = fp_row_in(cs->conflict, C, &dc->conflict);
    return n;
}
// one scenario's node table as inputs (five rows, in this order)
static inline int fp_node_rows(const fp_nodes *ns, fp_nodes *dn, fp_row *r) {
    const size_t N = ns->n;
    *dn = *ns;
    int n = 0;
    r[n++] = fp_row_in(ns->cpu_free, N, &dn->cpu_free);
    r[n++] = fp_row_in(ns->mem_free, N, &dn->mem_free);
    r[n++] = fp_row_in(ns->labels, N, &dn->labels);
    r[n++] = fp_row_in(ns->conflict_used, N, &dn->conflict_used);
    r[n++] = fp_row_in(ns->schedulable, N, &dn->schedulable);
    return n;
}
// both tables: the container rows, then the node rows
static inline int fp_tables_rows(const fp_containers *cs, const fp_nodes *ns, fp_containers *dc, fp_nodes *dn,
                                 fp_row *r) {
    const int n = fp_cont_rows(cs, dc, r);
    return n + fp_node_rows(ns, dn, r + n);
}

// fp_drain_sweep: the tables, the live plan, the candidate groups, the counts; then the three results
struct fp_drain_dev {
    fp_containers cs;
    fp_nodes ns;
    const uint32_t *assign, *group, *node_count;
    uint32_t *assign_out, *summary;
    uint8_t *reason_out;
};
static inline int fp_drain_rows(const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                const uint32_t *group, uint32_t n_cand, const uint32_t *node_count,
                                uint32_t *assign_out, uint8_t *reason_out, uint32_t *summary_out, fp_drain_dev *d,
                                fp_row *r) {
    const size_t C = cs->n, N = ns->n;
    int n = fp_tables_rows(cs, ns, &d->cs, &d->ns, r);
    r[n++] = fp_row_in(assign, C, &d->assign);
    r[n++] = fp_row_in(group, N, &d->group);
    r[n++] = fp_row_in(node_count, N, &d->node_count);
    r[n++] = fp_row_out(assign_out, C, &d->assign_out);
    r[n++] = fp_row_out(reason_out, C, &d->reason_out);
    r[n++] = fp_row_out(summary_out, (size_t)n_cand * FP_DRAIN_WORDS, &d->summary);
    return n;
}

// fp_drain_sweep_policy (SPEC.md 2.15): fp_drain_sweep's rows, then the domains (absent without a constraint)
// and the two further results the caller may ask for.  relax_mask stays on the host
struct fp_drain_policy_dev {
    const uint32_t *domain;
    uint8_t *hops_out;
    uint32_t *policy_out;
};
static inline int fp_drain_policy_rows(const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                       const uint32_t *group, uint32_t n_cand, const uint32_t *node_count,
                                       const uint32_t *domain, uint32_t *assign_out, uint8_t *reason_out,
                                       uint8_t *hops_out, uint32_t *summary_out, uint32_t *policy_out, fp_drain_dev *d,
                                       fp_drain_policy_dev *dp, fp_row *r) {
    int n = fp_drain_rows(cs, ns, assign, group, n_cand, node_count, assign_out, reason_out, summary_out, d, r);
    r[n++] = fp_row_in(domain, (size_t)ns->n, &dp->domain);
    r[n++] = fp_row_opt(hops_out, (size_t)cs->n, &dp->hops_out);
    r[n++] = fp_row_opt(policy_out, (size_t)n_cand * FP_DRAIN_POLICY_WORDS, &dp->policy_out);
    return n;
}

// fp_shrink_sweep (SPEC.md 2.16): the tables, the live plan, the release orders, the counts; then the four results
struct fp_shrink_dev {
    fp_containers cs;
    fp_nodes ns;
    const uint32_t *assign, *try_order, *node_count;
    uint32_t *assign_out, *blocker_out, *summary;
    uint8_t *state_out;
};
static inline int fp_shrink_rows(const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                 const uint32_t *try_order, uint32_t n_var, uint32_t n_try, const uint32_t *node_count,
                                 uint32_t *assign_out, uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out,
                                 fp_shrink_dev *d, fp_row *r) {
    const size_t C = cs->n, N = ns->n, V = n_var;
    int n = fp_tables_rows(cs, ns, &d->cs, &d->ns, r);
    r[n++] = fp_row_in(assign, C, &d->assign);
    r[n++] = fp_row_in(try_order, V * n_try, &d->try_order);
    r[n++] = fp_row_in(node_count, N, &d->node_count);
    r[n++] = fp_row_out(assign_out, V * C, &d->assign_out);
    r[n++] = fp_row_out(state_out, V * N, &d->state_out);
    r[n++] = fp_row_opt(blocker_out, V * N, &d->blocker_out);
    r[n++] = fp_row_out(summary_out, V * FP_SHRINK_WORDS, &d->summary);
    return n;
}

// fp_shrink_sweep_policy (SPEC.md 2.17): fp_shrink_sweep's rows, then the domains (absent without a constraint)
// and the three further results the caller may ask for.  relax_mask stays on the host
struct fp_shrink_policy_dev {
    const uint32_t *domain;
    uint8_t *hops_out, *blocker_reason_out;
    uint32_t *policy_out;
};
static inline int fp_shrink_policy_rows(const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                        const uint32_t *try_order, uint32_t n_var, uint32_t n_try,
                                        const uint32_t *node_count, const uint32_t *domain, uint32_t *assign_out,
                                        uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out,
                                        uint8_t *hops_out, uint8_t *blocker_reason_out, uint32_t *policy_out,
                                        fp_shrink_dev *d, fp_shrink_policy_dev *dp, fp_row *r) {
    const size_t V = n_var;
    int n = fp_shrink_rows(cs, ns, assign, try_order, n_var, n_try, node_count, assign_out, state_out, blocker_out,
                           summary_out, d, r);
    r[n++] = fp_row_in(domain, (size_t)ns->n, &dp->domain);
    r[n++] = fp_row_opt(hops_out, V * cs->n, &dp->hops_out);
    r[n++] = fp_row_opt(blocker_reason_out, V * ns->n, &dp->blocker_reason_out);
    r[n++] = fp_row_opt(policy_out, V * FP_SHRINK_POLICY_WORDS, &dp->policy_out);
    return n;
}

// fp_rebalance_sweep (SPEC.md 2.19): the tables, the live plan, the victim orders with their budgets, the counts
// and the domains (each absent when the caller gives none); then the four results.  relax_mask stays on the host
struct fp_rebalance_dev {
    fp_containers cs;
    fp_nodes ns;
    const uint32_t *assign, *victim_order, *max_moves, *node_count, *domain;
    uint32_t *assign_out, *summary;
    uint8_t *hops_out, *reason_out;
};
static inline int fp_rebalance_rows(const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                    const uint32_t *victim_order, uint32_t n_var, uint32_t n_try,
                                    const uint32_t *max_moves, const uint32_t *node_count, const uint32_t *domain,
                                    uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out,
                                    fp_rebalance_dev *d, fp_row *r) {
    const size_t C = cs->n, N = ns->n, V = n_var;
    int n = fp_tables_rows(cs, ns, &d->cs, &d->ns, r);
    r[n++] = fp_row_in(assign, C, &d->assign);
    r[n++] = fp_row_in(victim_order, V * n_try, &d->victim_order);
    r[n++] = fp_row_in(max_moves, V, &d->max_moves);
    r[n++] = fp_row_in(node_count, N, &d->node_count);
    r[n++] = fp_row_in(domain, N, &d->domain);
    r[n++] = fp_row_out(assign_out, V * C, &d->assign_out);
    r[n++] = fp_row_opt(hops_out, V * C, &d->hops_out);
    r[n++] = fp_row_opt(reason_out, V * C, &d->reason_out);
    r[n++] = fp_row_out(summary_out, V * FP_REBAL_WORDS, &d->summary);
    return n;
}

// fp_grow_sweep: the requests, the reasons (absent without a mask), the templates; then the two results
struct fp_grow_dev {
    fp_containers cs;
    const uint8_t *reason;
    const uint32_t *t_cpu, *t_mem, *t_labels, *t_max;
    uint32_t *summary, *assign_out;
};
// the requests and their reasons (absent without a mask): what both grow lists begin with
static inline int fp_grow_pending(const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask, fp_grow_dev *d,
                                  fp_row *r) {
    int n = fp_cont_rows(cs, &d->cs, r);
    r[n++] = fp_row_in(reason_mask ? reason : nullptr, (size_t)cs->n, &d->reason);
    return n;
}
static inline int fp_grow_rows(const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask, uint32_t n_cand,
                               const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                               const uint32_t *t_max, uint32_t *summary_out, uint32_t *assign_out, fp_grow_dev *d,
                               fp_row *r) {
    const size_t C = cs->n, K = n_cand;
    int n = fp_grow_pending(cs, reason, reason_mask, d, r);
    r[n++] = fp_row_in(t_cpu, K, &d->t_cpu);
    r[n++] = fp_row_in(t_mem, K, &d->t_mem);
    r[n++] = fp_row_in(t_labels, K, &d->t_labels);
    r[n++] = fp_row_in(t_max, K, &d->t_max);
    r[n++] = fp_row_out(summary_out, K * FP_GROW_WORDS, &d->summary);
    r[n++] = fp_row_opt(assign_out, K * C, &d->assign_out);
    return n;
}

// fp_grow_sweep_policy (SPEC.md 2.18): fp_grow_sweep's inputs, the live table with its counts and domains, the
// templates' domains (both domain rows absent without a constraint); then the five results.  relax_mask, quota
// and quota_used stay on the host
struct fp_grow_policy_dev {
    fp_nodes ns;
    const uint32_t *node_count, *domain, *t_domain;
    uint32_t *policy_out;
    uint8_t *hops_out, *reason_out;
};
static inline int fp_grow_policy_rows(const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                                      const fp_nodes *ns, const uint32_t *node_count, uint32_t n_cand,
                                      const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                                      const uint32_t *t_max, const uint32_t *domain, const uint32_t *t_domain,
                                      uint32_t *summary_out, uint32_t *policy_out, uint32_t *assign_out,
                                      uint8_t *hops_out, uint8_t *reason_out, fp_grow_dev *d, fp_grow_policy_dev *dp,
                                      fp_row *r) {
    const size_t C = cs->n, N = ns->n, K = n_cand;
    int n = fp_grow_pending(cs, reason, reason_mask, d, r);
    n += fp_node_rows(ns, &dp->ns, r + n);
    r[n++] = fp_row_in(node_count, N, &dp->node_count);
    r[n++] = fp_row_in(domain, N, &dp->domain);
    r[n++] = fp_row_in(t_cpu, K, &d->t_cpu);
    r[n++] = fp_row_in(t_mem, K, &d->t_mem);
    r[n++] = fp_row_in(t_labels, K, &d->t_labels);
    r[n++] = fp_row_in(t_max, K, &d->t_max);
    r[n++] = fp_row_in(t_domain, K, &dp->t_domain);
    r[n++] = fp_row_out(summary_out, K * FP_GROW_WORDS, &d->summary);
    r[n++] = fp_row_opt(policy_out, K * FP_GROW_POLICY_WORDS, &dp->policy_out);
    r[n++] = fp_row_opt(assign_out, K * C, &d->assign_out);
    r[n++] = fp_row_opt(hops_out, K * C, &dp->hops_out);
    r[n++] = fp_row_opt(reason_out, K * C, &dp->reason_out);
    return n;
}
