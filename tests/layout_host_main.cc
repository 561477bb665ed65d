// The arena layout arithmetic (fleetflow_amd/csrc/fp_layout.h) and the row lists of the host-pointer entry points
// (fp_rows.h), checked without a GPU.  tests/test_layout_host.py builds this with -fsanitize=address,undefined
// and runs it: a layout that reaches past the total it reports is a heap overflow here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../fleetflow_amd/csrc/fp_rows.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// Lays the rows out, stages them into a heap block of exactly the reported total the way fp_ctx.hip does
// (inputs copied in, every taken row written over its full length with its pad) and checks the layout's
// properties.  Returns the total.
static size_t stage_and_check(const fp_row *r, int n) {
    size_t off[FP_MAX_ROWS];
    CHECK(n <= FP_MAX_ROWS);
    const size_t total = fp_rows_layout(r, n, 0, off);
    char *arena = (char *)malloc(total ? total : 1);
    fp_rows_point(r, n, arena, off);
    // the same rule the takes use: one fp_take_end per taken row reproduces every offset and the total
    size_t top = 0, prev_end = 0;
    for (int i = 0; i < n; ++i) {
        char *d = (char *)*r[i].dev;
        if (!fp_row_taken(r[i])) {
            CHECK(d == nullptr);  // a null input takes nothing and yields a null device pointer
            continue;
        }
        const size_t len = r[i].bytes + FP_STAGE_PAD;
        const size_t end = fp_take_end(top, len);
        CHECK(d == arena + (end - len));
        CHECK(off[i] % 256 == 0);
        CHECK(off[i] >= prev_end);  // disjoint, in the order of the rows
        CHECK(off[i] + len <= total);
        if (r[i].in) memcpy(d, r[i].in, r[i].bytes);
        else memset(d, 0xA5, r[i].bytes);
        memset(d + r[i].bytes, 0, FP_STAGE_PAD);
        prev_end = off[i] + len;
        top = end;
    }
    CHECK(top == total);  // the total is the end of the last take
    CHECK(prev_end == total);
    free(arena);
    return total;
}

static void test_generic() {
    std::vector<uint32_t> a(70, 7u), b(1, 9u), e(1, 0u);
    std::vector<uint8_t> s(9, 1u);
    const uint32_t *da = nullptr, *dnull = (const uint32_t *)16, *dempty = nullptr, *db = nullptr;
    const uint8_t *ds = nullptr;
    uint32_t *dout = nullptr, *dopt = (uint32_t *)16, *dopt2 = nullptr, *dio = nullptr;
    uint32_t out[3], opt2[5];
    const fp_row rows[] = {
        fp_row_in(a.data(), a.size(), &da),
        fp_row_in((const uint32_t *)nullptr, 1000, &dnull),  // null: nothing, whatever the length says
        fp_row_in(e.data(), 0, &dempty),                     // non-null of length 0: its own address
        fp_row_in(s.data(), s.size(), &ds),
        fp_row_io(b.data(), b.size(), &db),
        fp_row_out(out, 3, &dout),
        fp_row_opt((uint32_t *)nullptr, 100, &dopt),  // an optional result nobody asked for
        fp_row_opt(opt2, 5, &dopt2),
        fp_row_out((uint32_t *)nullptr, 2, &dio),  // a result the kernels write that is not copied back
    };
    const size_t total = stage_and_check(rows, (int)(sizeof rows / sizeof *rows));
    CHECK(dnull == nullptr && dopt == nullptr);
    CHECK(dempty != nullptr && (const void *)dempty != (const void *)da && (const void *)dempty != (const void *)ds);
    CHECK(dio != nullptr);
    // 7 taken rows: offsets 0, 512, 768, 1024, 1280, 1536, 1792; the last is 2 * 4 + 4 bytes long
    CHECK(total == 1792 + 12);
    CHECK(fp_align256(0) == 0 && fp_align256(1) == 256 && fp_align256(256) == 256 && fp_align256(257) == 512);
    CHECK(fp_take_end(0, 4) == 4 && fp_take_end(4, 0) == 256 && fp_take_end(255, 10) == 266);
}

// the byte formulas the entry points reserved by before their rows sized the arena
static size_t old_policy_formula(size_t S, size_t C, size_t N) {
    const size_t SC = S * C, SN = S * N;
    return SC * (4 * 6 + 1 + 1 + 1) + SN * (4 * 6 + 1) +
           S * (8 + 4 + 4 + 4 + 4 * FP_FALLBACK_MAX_HOPS + 4 + 2 * 4 * FP_QUOTA_DIMS) + 28 * 256;
}
static size_t old_drain_formula(size_t C, size_t N, size_t n_cand) {
    const size_t R = n_cand * FP_DRAIN_WORDS;
    return C * 25 + N * 25 + R * 4 + 20 * 256;
}

// ---- the sweep lists and the re-plan list ----------------------------------------------------------------------
// where every row of a list starts, in units of 256 bytes (-1: the row takes nothing); returns the total
static size_t row_offsets(const fp_row *r, int n, long *at) {
    size_t off[FP_MAX_ROWS];
    const size_t total = fp_rows_layout(r, n, 0, off);
    for (int i = 0; i < n; ++i) at[i] = fp_row_taken(r[i]) ? (long)(off[i] / 256) : -1;
    return total;
}

// The order of the rows is the arena layout: the offsets of every list at S = 2, C = 70, N = 9 (2 variants of 9
// tries, 3 templates, every option given), recorded from the lists as they were when each entry point had its own.
struct pinned_list {
    const char *name;
    int n;
    long at[FP_MAX_ROWS];
};
static const pinned_list PINNED[] = {
    {"drain", 15, {0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 15, 16, 17, 19, 20}},
    {"drain_policy", 18, {0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 15, 16, 17, 19, 20, 22, 23, 24}},
    {"shrink", 16, {0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 15, 16, 17, 20, 21, 22}},
    {"shrink_policy", 20, {0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 15, 16, 17, 20, 21, 22, 23, 24, 25, 26}},
    {"grow", 11, {0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14}},
    {"grow_policy", 22, {0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 27, 28}},
    {"replan", 27, {0,  3,  6,  9,  12, 15, 16, 17, 18, 19, 20, 21, 22, 23,
                    24, 25, 26, 27, 28, 29, 32, 33, 34, 35, 36, 39, 40}},
};

static void check_pinned(const char *name, const fp_row *r, int n, bool pinned) {
    long at[FP_MAX_ROWS];
    row_offsets(r, n, at);
    if (!pinned) return;
    printf("order %s:", name);
    for (int i = 0; i < n; ++i) printf(" %ld", at[i]);
    printf("\n");
    for (const pinned_list &p : PINNED) {
        if (strcmp(p.name, name)) continue;
        CHECK(p.n == n);
        for (int i = 0; i < n && i < p.n; ++i) CHECK(p.at[i] == at[i]);
        return;
    }
    CHECK(!"a list without a pinned order");
}

static void test_sweep_lists(uint32_t S, uint32_t C, uint32_t N, fp_batch *b, const fp_policy_opts *o,
                             const fp_containers *cs, const fp_nodes *ns) {
    const bool pin = S == 2 && C == 70 && N == 9;
    const uint32_t V = 2, K = 3, n_try = N;
    const size_t SC = (size_t)S * C;
    std::vector<uint32_t> in((SC > 2 * (size_t)N ? SC : 2 * (size_t)N) + 64, 1u);  // every u32 input reads from this
    std::vector<uint8_t> in8(C + 1, 1u);
    uint32_t o32[1];  // results are never written through their host pointer here: non-null is all they need
    uint8_t o8[1];
    fp_row rows[FP_MAX_ROWS], plain[FP_MAX_ROWS];
    long at[FP_MAX_ROWS], at_plain[FP_MAX_ROWS];

    // drain: every option, then the policy list without a guarantee against the plain list
    fp_drain_dev dd, dd0;
    fp_drain_policy_dev dp;
    int n = fp_drain_policy_rows(cs, ns, in.data(), in.data(), N, in.data(), in.data(), o32, o8, o8, o32, o32, &dd, &dp,
                                 rows);
    CHECK(n == 18);
    stage_and_check(rows, n);
    CHECK(dd.cs.conflict && dd.ns.cpu_free && dd.assign && dd.group && dd.node_count && dd.assign_out && dd.reason_out &&
          dd.summary && dp.domain && dp.hops_out && dp.policy_out);
    check_pinned("drain_policy", rows, n, pin);
    n = fp_drain_policy_rows(cs, ns, in.data(), in.data(), N, in.data(), nullptr, o32, o8, nullptr, o32, nullptr, &dd, &dp,
                             rows);
    int n0 = fp_drain_rows(cs, ns, in.data(), in.data(), N, in.data(), o32, o8, o32, &dd0, plain);
    CHECK(n == 18 && n0 == 15);
    CHECK(row_offsets(rows, n, at) == row_offsets(plain, n0, at_plain));
    for (int i = 0; i < n0; ++i) CHECK(at[i] == at_plain[i] && rows[i].bytes == plain[i].bytes && at[i] >= 0);
    for (int i = n0; i < n; ++i) CHECK(at[i] == -1);
    stage_and_check(rows, n);
    CHECK(!dp.domain && !dp.hops_out && !dp.policy_out && dd.summary);
    check_pinned("drain", plain, n0, pin);

    // shrink
    fp_shrink_dev sd, sd0;
    fp_shrink_policy_dev sp;
    n = fp_shrink_rows(cs, ns, in.data(), in.data(), V, n_try, in.data(), o32, o8, o32, o32, &sd, rows);
    CHECK(n == 16);
    stage_and_check(rows, n);
    CHECK(sd.cs.cpu_m && sd.ns.schedulable && sd.assign && sd.try_order && sd.node_count && sd.assign_out &&
          sd.state_out && sd.blocker_out && sd.summary);
    check_pinned("shrink", rows, n, pin);
    n = fp_shrink_policy_rows(cs, ns, in.data(), in.data(), V, n_try, in.data(), in.data(), o32, o8, o32, o32, o8, o8, o32,
                              &sd, &sp, rows);
    CHECK(n == 20);
    stage_and_check(rows, n);
    CHECK(sd.cs.cpu_m && sd.ns.schedulable && sd.assign && sd.try_order && sd.node_count && sd.assign_out &&
          sd.state_out && sd.blocker_out && sd.summary && sp.domain && sp.hops_out && sp.blocker_reason_out &&
          sp.policy_out);
    check_pinned("shrink_policy", rows, n, pin);
    n = fp_shrink_policy_rows(cs, ns, in.data(), in.data(), V, n_try, in.data(), nullptr, o32, o8, o32, o32, nullptr,
                              nullptr, nullptr, &sd, &sp, rows);
    n0 = fp_shrink_rows(cs, ns, in.data(), in.data(), V, n_try, in.data(), o32, o8, o32, o32, &sd0, plain);
    CHECK(n == 20 && n0 == 16);
    CHECK(row_offsets(rows, n, at) == row_offsets(plain, n0, at_plain));
    for (int i = 0; i < n0; ++i) CHECK(at[i] == at_plain[i] && rows[i].bytes == plain[i].bytes && at[i] >= 0);
    for (int i = n0; i < n; ++i) CHECK(at[i] == -1);
    stage_and_check(rows, n);
    CHECK(!sp.domain && !sp.hops_out && !sp.blocker_reason_out && !sp.policy_out && sd.summary);

    // grow
    fp_grow_dev gd, gd0;
    fp_grow_policy_dev gp;
    n = fp_grow_rows(cs, in8.data(), 2u, K, in.data(), in.data(), in.data(), in.data(), o32, o32, &gd, rows);
    CHECK(n == 11);
    stage_and_check(rows, n);
    CHECK(gd.cs.cpu_m && gd.cs.conflict && gd.reason && gd.t_cpu && gd.t_mem && gd.t_labels && gd.t_max && gd.summary &&
          gd.assign_out);
    check_pinned("grow", rows, n, pin);
    n = fp_grow_policy_rows(cs, in8.data(), 2u, ns, in.data(), K, in.data(), in.data(), in.data(), in.data(), in.data(),
                            in.data(), o32, o32, o32, o8, o8, &gd, &gp, rows);
    CHECK(n == 22);
    stage_and_check(rows, n);
    CHECK(gd.cs.cpu_m && gd.reason && gp.ns.cpu_free && gp.ns.schedulable && gp.node_count && gp.domain && gd.t_cpu &&
          gd.t_max && gp.t_domain && gd.summary && gp.policy_out && gd.assign_out && gp.hops_out && gp.reason_out);
    check_pinned("grow_policy", rows, n, pin);
    // no live table and no policy option: the container, reason, template and result rows lie where fp_grow_rows
    // puts them
    fp_nodes none = {};
    n = fp_grow_policy_rows(cs, in8.data(), 2u, &none, nullptr, K, in.data(), in.data(), in.data(), in.data(), nullptr,
                            nullptr, o32, nullptr, o32, nullptr, nullptr, &gd, &gp, rows);
    n0 = fp_grow_rows(cs, in8.data(), 2u, K, in.data(), in.data(), in.data(), in.data(), o32, o32, &gd0, plain);
    CHECK(n == 22 && n0 == 11);
    CHECK(row_offsets(rows, n, at) == row_offsets(plain, n0, at_plain));
    const int same[11] = {0, 1, 2, 3, 4, 12, 13, 14, 15, 17, 19};  // where the eleven rows stand among the 22
    for (int i = 0; i < n0; ++i) CHECK(at[same[i]] == at_plain[i] && rows[same[i]].bytes == plain[i].bytes && at_plain[i] >= 0);
    int taken = 0;
    for (int i = 0; i < n; ++i) taken += at[i] >= 0;
    CHECK(taken == n0);
    stage_and_check(rows, n);
    CHECK(gd.cs.cpu_m && gd.t_max && gd.summary && gd.assign_out && !gp.ns.cpu_free && !gp.node_count && !gp.policy_out);

    // re-plan with every policy option
    b->level = in.data();
    fp_batch d;
    fp_policy_opts dopt;
    fp_replan_dev dr;
    n = fp_replan_rows(b, o, in.data(), o8, o32, &d, &dopt, &dr, rows);
    CHECK(n == 27);
    stage_and_check(rows, n);
    CHECK(d.cpu_m && d.level && d.schedulable && d.assign && d.reason && d.cost && dopt.strategy && dopt.preferred &&
          dopt.node_count && dopt.domain && dopt.max_skew && dopt.relax_mask && dopt.n_hops && dopt.quota &&
          dopt.quota_used && dopt.hops && dopt.quota_why && dr.prev && dr.change && dr.summary);
    check_pinned("replan", rows, n, pin);
}

static void test_entry_points(uint32_t S, uint32_t C, uint32_t N) {
    const size_t SC = (size_t)S * C, SN = (size_t)S * N;
    const size_t big = (SC > SN ? SC : SN) + (size_t)S * 8 + 64;
    std::vector<uint32_t> w(big, 1u);  // every u32 array of the call reads from / writes to this
    std::vector<uint8_t> by(big, 1u);
    std::vector<uint64_t> cost(S + 1);
    fp_batch b = {};
    b.n_scen = S; b.n_containers = C; b.n_nodes = N;
    b.cpu_m = b.mem_mib = b.req_labels = b.conflict = b.level = b.labels = w.data();
    b.cpu_free = b.mem_free = b.conflict_used = w.data();
    b.schedulable = by.data();
    b.assign = w.data(); b.reason = by.data(); b.cost = cost.data();
    fp_policy_opts o;  // fp_place_batch_policy_quota with every option given
    o.strategy = o.preferred = o.domain = o.max_skew = o.relax_mask = o.n_hops = o.quota = w.data();
    o.node_count = o.quota_used = w.data();
    o.hops = o.quota_why = by.data();
    fp_row rows[FP_MAX_ROWS];
    fp_batch d;
    fp_policy_opts dopt;
    int n = fp_batch_rows(&b, &o, &d, &dopt, rows);
    CHECK(n == 24);
    size_t total = stage_and_check(rows, n);
    printf("policy S=%u C=%u N=%u: rows %zu, formula %zu\n", S, C, N, total, old_policy_formula(S, C, N));
    CHECK(total <= old_policy_formula(S, C, N));
    CHECK(d.cpu_m && d.schedulable && d.assign && d.reason && d.cost && dopt.strategy && dopt.quota_used && dopt.hops &&
          dopt.quota_why);
    // first fit: the ten inputs and the three results, no policy row; the level is optional
    b.level = nullptr;
    n = fp_batch_rows(&b, nullptr, &d, nullptr, rows);
    CHECK(n == 13);
    stage_and_check(rows, n);
    CHECK(d.level == nullptr && d.cpu_m != nullptr);

    fp_containers cs = {};
    fp_nodes ns = {};
    cs.n = C; ns.n = N;
    cs.cpu_m = cs.mem_mib = cs.req_labels = cs.conflict = w.data();
    ns.cpu_free = ns.mem_free = ns.conflict_used = w.data();
    ns.labels = w.data(); ns.schedulable = by.data();
    fp_drain_dev dd;
    std::vector<uint32_t> assign_out(C + 1), summary((size_t)N * FP_DRAIN_WORDS + 1);
    n = fp_drain_rows(&cs, &ns, w.data(), w.data(), N, w.data(), assign_out.data(), by.data(), summary.data(), &dd, rows);
    CHECK(n == 15);
    total = stage_and_check(rows, n);
    printf("drain C=%u N=%u n_cand=%u: rows %zu, formula %zu\n", C, N, N, total, old_drain_formula(C, N, N));
    CHECK(total <= old_drain_formula(C, N, N));
    CHECK(dd.cs.cpu_m && dd.ns.schedulable && dd.assign && dd.group && dd.node_count && dd.assign_out && dd.reason_out &&
          dd.summary);
    test_sweep_lists(S, C, N, &b, &o, &cs, &ns);
}

int main() {
    test_generic();
    test_entry_points(2, 70, 9);
    test_entry_points(3, 3000, 700);
    test_entry_points(1, 1, 1);
    test_entry_points(1, 0, 0);
    test_entry_points(5, 255, 8192);  // odd lengths: every row pays its alignment
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("layout ok\n");
    return 0;
}
