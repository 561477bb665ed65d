// fp_layout.h -- the layout arithmetic of the two bump arenas (fp_ws_take, fp_stage_take) and of the staged
// buffers of a host-pointer call (fp_ctx.hip).  Free of HIP, so that tests/test_layout_host.py checks it on
// the CPU: what a call reserves is computed here from the same rows its takes and copies walk, never from a
// byte formula kept next to them.
#pragma once
#include <stddef.h>

static inline size_t fp_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// where a take of `bytes` ends in an arena whose top is `top`; it starts at fp_align256(top)
static inline size_t fp_take_end(size_t top, size_t bytes) { return fp_align256(top) + bytes; }

// every staged buffer is taken 4 bytes longer than its array (a kernel may read one word past a row's end)
constexpr size_t FP_STAGE_PAD = 4;

// One device buffer of a host-pointer call.  A row takes `bytes + FP_STAGE_PAD` when it has a host source or
// `take` is set; otherwise (a null input, an optional output nobody asked for) it takes nothing and *dev is
// null.  The order of the rows is the order of the takes: the layout of the staging arena.
struct fp_row {
    const void *in;  // host source, null: nothing is copied in
    void *out;       // host destination, null: nothing is copied back
    size_t bytes;
    void **dev;      // receives the device pointer
    bool take;       // takes its place without a host source (an output)
};

static inline bool fp_row_taken(const fp_row &r) { return r.in != nullptr || r.take; }

// off[i] = where row i starts in an arena whose top is `top` (unset for a row that takes nothing); returns the
// top behind the last take
static inline size_t fp_rows_layout(const fp_row *r, int n, size_t top, size_t *off) {
    for (int i = 0; i < n; ++i) {
        if (!fp_row_taken(r[i])) continue;
        off[i] = fp_align256(top);
        top = fp_take_end(top, r[i].bytes + FP_STAGE_PAD);
    }
    return top;
}

// hands out the device pointers of rows laid out at off[] from `base`: null for a row that takes nothing
static inline void fp_rows_point(const fp_row *r, int n, char *base, const size_t *off) {
    for (int i = 0; i < n; ++i) *r[i].dev = fp_row_taken(r[i]) ? base + off[i] : nullptr;
}
