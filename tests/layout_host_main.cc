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
