// extern "C" entry points of the rasterizer's frame (see include/goi_raster.h): workspace layout, stage orchestration on the
// caller's HIP stream, read-back tickets, options, per-stage event timing -- and the one definition of what every entry
// refuses a call with (entry.h).  A stand-alone family's entries are in the family's own unit, and so is an entry that drives one
// kernel family of the rasterizer directly (tests, diagnostics).  The goi_raster_debug_* entries left here belong to no single
// unit: the backward blend's drives three, the others answer questions about the layouts.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "common.h"
#include "entry.h"

namespace goi {

// entry.h: the refusals of every unit's entries end in this one thread_local message
static thread_local std::string g_err;

int fail(const char* where, hipError_t e) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return -1;
}
int fail(const std::string& msg) {
    g_err = msg;
    return -1;
}
int check_workspace(const std::string& fn, const void* ws, const char* what) {
    if (!ws) return fail(fn + ": NULL " + what);
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(fn + ": " + what + " must be 256-byte aligned");
    return 0;
}

namespace {

// ---- per-stage timing -------------------------------------------------------------------------
struct StageEvents {
    int stage;
    hipEvent_t a, b;
};
// (process-wide and shared by every calling thread: the mask is atomic, the event lists sit behind a mutex.  Stage timing
// is a single-device measurement aid: events are created on whichever device is current when they are first needed.)
std::atomic<unsigned> g_profile_mask{0};  // bit i = record HIP events around GOI_STAGE_i
std::mutex g_profile_mu;
std::vector<StageEvents> g_events;
std::vector<hipEvent_t> g_pool;

hipEvent_t get_event() {
    {
        std::lock_guard<std::mutex> lk(g_profile_mu);
        if (!g_pool.empty()) {
            hipEvent_t e = g_pool.back();
            g_pool.pop_back();
            return e;
        }
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct StageTimer {
    hipStream_t s;
    bool on;
    StageEvents ev{};
    StageTimer(int stage, hipStream_t st) : s(st), on((g_profile_mask.load(std::memory_order_relaxed) >> stage) & 1u) {
        if (on) {
            ev.stage = stage;
            ev.a = get_event();
            ev.b = get_event();
            (void)hipEventRecord(ev.a, s);
        }
    }
    ~StageTimer() {
        if (on) {
            (void)hipEventRecord(ev.b, s);
            std::lock_guard<std::mutex> lk(g_profile_mu);
            g_events.push_back(ev);
        }
    }
};

int check_stage(const GoiRasterScene& sc, hipStream_t s, const char* name) {
    if (!sc.debug) return 0;
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(name, e);
    return 0;
}

int validate(const GoiRasterScene* sc, bool need_sem, bool need_opacity = true) {
    if (!sc) return fail("scene is NULL");
    if (sc->P < 0 || sc->W <= 0 || sc->H <= 0) return fail("bad P/W/H");
    if (sc->S < 1 || sc->S > 32) return fail("semantic channels S must be in 1..32");
    if (sc->P == 0) return 0;
    if (need_opacity && !sc->opacities) return fail("opacities is NULL");
    if (!sc->means3D || !sc->viewmatrix || !sc->projmatrix || !sc->campos || !sc->bg)
        return fail("a required input pointer is NULL");
    if (need_sem && !sc->semantics) return fail("semantics is required (the reference dereferences it unconditionally)");
    if (sc->semantics && (sc->S & 3) == 0 && (reinterpret_cast<uintptr_t>(sc->semantics) & 15u) != 0)
        return fail("semantics must be 16-byte aligned when S is a multiple of 4 (its rows are moved as 16-byte words)");
    if ((sc->shs == nullptr) == (sc->colors_precomp == nullptr))
        return fail("Please provide excatly one of either SHs or precomputed colors!");
    // (an SH row whose 3 M floats are a whole number of 16-byte words -- M = 4, 8, 12, 16 -- is moved as such by both per-Gaussian
    // kernels: preprocess_fwd.hip, row16 / preprocess_bwd.hip, the hoist)
    if (sc->shs && (3 * sc->M) % 4 == 0 && (reinterpret_cast<uintptr_t>(sc->shs) & 15u) != 0)
        return fail("shs must be 16-byte aligned when 3 M is a multiple of 4 (its rows are moved as 16-byte words)");
    if (((sc->scales == nullptr || sc->rotations == nullptr) && sc->cov3D_precomp == nullptr) ||
        ((sc->scales != nullptr || sc->rotations != nullptr) && sc->cov3D_precomp != nullptr))
        return fail("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    // M <= 16: the kernels hold at most the 16 coefficients of degree 3, and preprocess_bwd stages 256 x (3M+1) floats
    // of dL/dSH in LDS (50 KB at M = 16) -- a larger M would only fail at backward time
    if (sc->shs && (sc->D < 0 || sc->D > 3 || sc->M < (sc->D + 1) * (sc->D + 1) || sc->M > 16))
        return fail("SH degree must be 0..3 and (D+1)^2 <= M <= 16");
    return 0;
}

// ---- read-back tickets ---------------------------------------------------------------------------
// num_rendered (and the "prefiltered" error flag) reach the host through a pinned copy of the frame's counters plus an
// event recorded right behind the copy.  A ticket is one such (pinned words, event) pair; they are pooled per DEVICE
// (events and pinned allocations belong to the device that was current when they were made) under a mutex, so
// concurrent callers on different streams / threads / GPUs each get their own.
constexpr int READBACK_HEAD_WORDS_MIN = 32;
struct Ticket {
    int dev = -1;
    uint32_t* pinned = nullptr;
    hipEvent_t ev = nullptr;
    bool busy = false;
    int capacity = 0;  // instances the frame's binning buffer holds (speculative frames); 0: exact frame
    bool head_only = false;  // only the first READBACK_HEAD_WORDS words were copied: num_rendered is counters[COUNTER_N]
    uint32_t* pinned_dev = nullptr;  // the same words as the device sees them (the pinned allocation is mapped)
    // STAMPED read-back (round 5): no copy and no event -- a wave of the forward blend stores the head words into the pinned
    // words and then, behind a system-scope fence, this use's sequence number into pinned[STAMP_WORD]; the host compares.
    // (An event recorded behind the blend cost the stream a ~5.6 us bubble per frame: rocprofv3 shows it as the only idle gap
    // of a training step, between render_fwd_k and the backward's first kernel.)
    uint32_t seq = 0;
    bool stamped = false;
    hipStream_t stream = nullptr;  // the stream the frame was enqueued on (the slow path of a blocking wait drains IT, nothing else)
};
constexpr int STAMP_WORD = HOST_STAMP_WORD;  // 33 (common.h: the blend kernels write it); the head is words 0..31, word 32 is a
                                            // num_rendered stripe of the full copy, which is never stamped
static_assert(STAMP_WORD >= READBACK_HEAD_WORDS_MIN && STAMP_WORD < COUNTER_WORDS, "stamp word inside the pinned block, outside the head");
// A read-back queued BEHIND the whole frame (speculative forward) finds num_rendered as one word (COUNTER_N, left by the
// listed-Gaussian compaction / the scan): 128 bytes travel instead of the 4 KB of striped partial counters -- which the
// runtime moved as three copy kernels per frame.
constexpr int READBACK_HEAD_WORDS = 32;
static_assert(COUNTER_N < READBACK_HEAD_WORDS && COUNTER_OVF < READBACK_HEAD_WORDS && NR_BASE >= READBACK_HEAD_WORDS, "head layout");
std::mutex g_ticket_mu;
std::vector<Ticket> g_tickets;
constexpr int MAX_TICKETS = 4096;

int ticket_acquire(int capacity) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail("hipGetDevice failed");
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    for (size_t i = 0; i < g_tickets.size(); i++)
        if (!g_tickets[i].busy && g_tickets[i].dev == dev) {
            g_tickets[i].busy = true;
            g_tickets[i].capacity = capacity;
            g_tickets[i].stamped = false;
            return (int)i;
        }
    if ((int)g_tickets.size() >= MAX_TICKETS)
        return fail("too many unresolved speculative forwards (goi_raster_ticket_result was never called for them)");
    Ticket t;
    t.dev = dev;
    GOI_HIP(hipHostMalloc(reinterpret_cast<void**>(&t.pinned), COUNTER_WORDS * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocCoherent));  // (coherent: a kernel's stores go straight to the host)
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&t.pinned_dev), t.pinned, 0) != hipSuccess) t.pinned_dev = nullptr;
    GOI_HIP(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    t.pinned[STAMP_WORD] = 0u;
    t.busy = true;
    t.capacity = capacity;
    g_tickets.push_back(t);
    return (int)g_tickets.size() - 1;
}

void ticket_release(int id) {
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    if (id >= 0 && id < (int)g_tickets.size()) g_tickets[id].busy = false;
}

// wait != 0: block until the frame's counters have arrived.  Returns 1 (done: *n = num_rendered), 0 (not yet; only
// when wait == 0) or -1 (error; the ticket is released).  A finished ticket is released.
int ticket_result(int id, int wait, long long* n, unsigned* frame_flags = nullptr) {
    Ticket t;
    {
        std::lock_guard<std::mutex> lk(g_ticket_mu);
        if (id < 0 || id >= (int)g_tickets.size() || !g_tickets[id].busy) return fail("invalid or already resolved ticket");
        t = g_tickets[id];
    }
    if (t.stamped) {
        // the blend's wave stores the head words, fences at system scope, then stores the stamp: an acquire load that sees
        // this use's sequence number sees the words
        auto arrived = [&]() { return __atomic_load_n(&t.pinned[STAMP_WORD], __ATOMIC_ACQUIRE) == t.seq; };
        if (!arrived()) {
            if (!wait) return 0;
            // spin politely; a frame is milliseconds.  After two seconds something is wrong with the device (or the frame
            // never ran): drain the FRAME'S STREAM and look once more -- never hang in here.  (Not the device: that would also
            // wait for every other stream, e.g. an RCCL collective whose peer needs this very host thread to make progress.)
            const auto t0 = std::chrono::steady_clock::now();
            int spins = 0;
            while (!arrived()) {
                if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(20));
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                    int cur = 0;
                    (void)hipGetDevice(&cur);
                    (void)hipSetDevice(t.dev);
                    const hipError_t e = hipStreamSynchronize(t.stream);
                    (void)hipSetDevice(cur);
                    if (e != hipSuccess || !arrived()) {
                        ticket_release(id);
                        return fail("the frame's counters never arrived (num_rendered read-back)", e);
                    }
                }
            }
        }
    } else if (wait) {
        hipError_t e = hipEventSynchronize(t.ev);
        if (e != hipSuccess) {
            ticket_release(id);
            return fail("hipEventSynchronize(num_rendered read-back)", e);
        }
    } else {
        hipError_t e = hipEventQuery(t.ev);
        if (e == hipErrorNotReady) return 0;
        if (e != hipSuccess) {
            ticket_release(id);
            return fail("hipEventQuery(num_rendered read-back)", e);
        }
    }
    unsigned long long total = 0;  // 64-bit: 32 stripes of up to 2^32-1 each
    if (t.head_only)
        total = t.pinned[COUNTER_N];
    else
        for (int i = 0; i < NR_STRIPES; i++) total += t.pinned[NR_BASE + NR_STRIDE * i];
    const bool filtered = t.pinned[1] != 0;
    // (a read-back queued behind the whole frame also carries the verdict of both sorts)
    const bool missorted = t.head_only && (t.pinned[COUNTER_SORTERR] != 0 || (t.pinned[COUNTER_OVF] & OVF_MISSORTED) != 0);
    if (frame_flags) *frame_flags = t.head_only ? t.pinned[COUNTER_OVF] : 0u;
    ticket_release(id);
    if (filtered) return fail("Point is filtered although prefiltered is set. This shouldn't happen!");
    if (missorted)
        return fail("a look-back of the radix sort timed out (preempted or shared GPU?): the frame's lists are not sorted; its "
                    "backward writes zero gradients, its image must not be used");
    if (total > 0x7FFFFFFFull) return fail("num_rendered overflows int32");
    *n = (long long)total;
    return 1;
}

// Front half of the forward -- everything that does not depend on num_rendered: preprocess, the read-back of the
// counters (queued BEFORE the depth sort: preprocess has already summed num_rendered, so a host that waits for it wakes
// up while the GPU is still sorting), depth sort, scan.  The scan also leaves num_rendered in counters[COUNTER_N] for
// the kernels of the back half.
int enqueue_readback(const GeomView& g, int ticket, hipStream_t s, bool head_only = false) {
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    Ticket& t = g_tickets[ticket];
    t.head_only = head_only;
    GOI_HIP(hipMemcpyAsync(t.pinned, g.counters, (head_only ? READBACK_HEAD_WORDS : COUNTER_WORDS) * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s));
    GOI_HIP(hipEventRecord(t.ev, s));
    return 0;
}

// ticket < 0: no read-back here (the speculative forward queues it behind the blend instead: nobody is waiting for it,
// and a device-to-host copy in the middle of the frame costs the stream a ~10 us bubble)
int enqueue_front(const GoiRasterScene& sc, GeomView& g, ImageView& im, int* radii, int ticket, const uint32_t** order_out,
                  hipStream_t s, const float* zcut, uint32_t* zlearn, const uint8_t* keep, int keep_invert) {
    const int P = sc.P;
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    // one memset: the counters and, right behind them, the control words of the depth sort
    const size_t depth_ctrl = g_options.sort_variant == 1 ? radix_sort_control_words((size_t)P, 0, 32) : 0;
    // (sizes rounded up to 256 bytes: the runtime splits a memset of any other size into two fill kernels; the few
    // extra words are scratch that is written before it is read)
    GOI_HIP(hipMemsetAsync(g.blk_coarse, 0,
                           round_up_256((size_t)(reinterpret_cast<char*>(g.scratch + depth_ctrl) -
                                                 reinterpret_cast<char*>(g.blk_coarse))), s));
    {
        StageTimer t(GOI_STAGE_PREPROCESS, s);
        launch_preprocess_fwd(sc, g, radii, im.ranges, gx * gy, s, zcut, zlearn, keep, keep_invert);  // also zeroes the tile ranges
    }
    if (check_stage(sc, s, "preprocess")) return -1;
    if (ticket >= 0 && enqueue_readback(g, ticket, s)) return -1;
    // Only the V LISTED Gaussians (tiles_touched > 0; half of the headline scene is culled) are depth-sorted: one small
    // pass compacts their (depth key, id) in id order -- the sort must stay stable -- and, reading the keys anyway, forms
    // the sort's digit histograms (its prologue kernel is skipped).  V lives on the device: grids cover P, the kernels stop
    // at counters[COUNTER_V]; the prefix sum over the depth order and emit walk the V listed Gaussians only.
    const bool onesweep = g_options.sort_variant == 1;
    const uint32_t* v_dev = g.counters + COUNTER_V;
    int order_idx;
    {
        StageTimer t(GOI_STAGE_DEPTH_SORT, s);
        launch_compact_listed(P, g, onesweep ? radix_sort_ghist(g.scratch, (size_t)P, 0, 32) : nullptr, /*pad=*/!onesweep, s);
        order_idx = radix_sort_pairs(g.sort_keys, g.sort_vals, (size_t)P, 0, 32, g.scratch, s, /*cleared=*/true,
                                     /*ghist_ready=*/onesweep, onesweep ? v_dev : nullptr, g.counters + COUNTER_SORTERR);
    }
    if (check_stage(sc, s, "depth sort")) return -1;
    *order_out = g.sort_vals[order_idx];
    {
        StageTimer t(GOI_STAGE_SCAN, s);
        exclusive_scan_u32(g.tiles_touched, *order_out, g.offsets, (size_t)P, nullptr, g.scratch, s, v_dev);
    }
    return 0;
}

// Back half: emit -> tile ranges -> tile sort, for a binning buffer that holds `cap` instances.  exact: cap IS
// num_rendered (known to the host); otherwise cap is a capacity and every kernel takes the count from
// counters[COUNTER_N], clamped to cap (an overflowed frame is truncated but memory-safe; the host redoes it).
int enqueue_back(const GoiRasterScene& sc, GeomView& g, ImageView& im, const BinView& bv_in, int cap, bool exact,
                 const uint32_t* order, const int* radii, const uint32_t** plist, hipStream_t s) {
    BinView bv = bv_in;  // (the caller hands bv_in.qmask to the blend itself)
    const int P = sc.P;
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    const uint32_t* n_dev = exact ? nullptr : g.counters + COUNTER_N;
    // Tile counting fused into emit (onesweep sort, tile grid small enough for an LDS histogram): the counts give
    // the tile ranges and the sort's digit histograms, so neither the keys nor the sorted keys are re-read for them.
    const bool counting = cap > 0 && g_options.sort_variant == 1 && emit_can_count_tiles(sc.W, sc.H);
    const int tile_bits = tile_key_bits((uint32_t)(gx * gy));
    {
        StageTimer t(GOI_STAGE_EMIT, s);
        if (counting) {
            // emit also clears the control words of the tile sort (status words, histograms, tickets): one launch less
            launch_emit_counting(P, sc.W, sc.H, g, order, radii, bv.keys[0], bv.vals[0], im.ranges, bv.scratch,
                                 radix_sort_control_words((size_t)cap, 0, tile_bits), (uint32_t)cap, s);
        }
        else if (cap > 0)
            launch_emit(P, sc.W, sc.H, g, order, radii, bv.keys[0], bv.vals[0], (uint32_t)cap, s);
    }
    if (check_stage(sc, s, "emit")) return -1;
    int fin;
    if (counting) {
        {
            StageTimer t(GOI_STAGE_RANGES, s);
            launch_tile_ranges_hist(sc.W, sc.H, im.ranges, radix_sort_ghist(bv.scratch, (size_t)cap, 0, tile_bits), g.counters, s);
        }
        StageTimer t(GOI_STAGE_TILE_SORT, s);
        fin = radix_sort_pairs(bv.keys, bv.vals, (size_t)cap, 0, tile_bits, bv.scratch, s, /*cleared=*/true,
                               /*ghist_ready=*/true, n_dev, g.counters + COUNTER_OVF);
    } else {
        {
            StageTimer t(GOI_STAGE_TILE_SORT, s);
            fin = radix_sort_pairs(bv.keys, bv.vals, (size_t)cap, 0, tile_bits, bv.scratch, s, false, false, n_dev,
                                   g.counters + COUNTER_OVF);
        }
        if (check_stage(sc, s, "tile sort")) return -1;
        StageTimer t(GOI_STAGE_RANGES, s);
        launch_ranges(cap, n_dev, bv.keys[fin], im.ranges, gx * gy, s);
    }
    if (check_stage(sc, s, "tile sort / ranges")) return -1;
    *plist = bv.vals[fin];
    return 0;
}

// The exact front end shared by goi_raster_forward and goi_raster_trace: the host waits for num_rendered (the one
// read-back of the reference, CR/rasterizer_impl.cu:285), sizes the binning workspace through the allocation callback
// and enqueues the back half while the GPU is still busy with the depth sort and the scan -- no idle gap on the device.
// Returns num_rendered (>= 0) and the final point list through *plist.
int geometry_and_binning(const GoiRasterScene& sc, GeomView& g, ImageView& im, goi_alloc_fn alloc, void* user,
                         int* radii, const uint32_t** plist, hipStream_t s, unsigned long long** qmask = nullptr,
                         const uint8_t* keep = nullptr, int keep_invert = 0) {
    const int ticket = ticket_acquire(0);
    if (ticket < 0) return -1;
    const uint32_t* order = nullptr;
    if (enqueue_front(sc, g, im, radii, ticket, &order, s, nullptr, nullptr, keep, keep_invert)) {
        ticket_release(ticket);
        return -1;
    }
    long long n64 = 0;
    if (ticket_result(ticket, 1, &n64) < 0) return -1;
    const int N = (int)n64;
    const size_t need = goi_raster_binning_bytes(N);
    char* bin_mem = static_cast<char*>(alloc(user, need));
    if (!bin_mem && need > 0) return fail("binning allocation callback returned NULL");
    BinView bv;
    binning_layout(N, bin_mem, &bv);
    if (qmask) *qmask = bv.qmask;
    if (enqueue_back(sc, g, im, bv, N, /*exact=*/true, order, radii, plist, s)) return -1;
    return N;
}

}  // namespace

thread_local Options g_options;
static Options g_shared_options;
static std::mutex g_options_mu;
void refresh_options() {
    std::lock_guard<std::mutex> lk(g_options_mu);
    g_options = g_shared_options;
}

// Which ping-pong buffer holds the tile-sorted list: a pure function of the pass count, so the
// backward can recompute it instead of storing it.
static int tile_sort_result_index(int W, int H, int N) {
    if (N <= 0) return 0;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int passes = (tile_key_bits((uint32_t)(gx * gy)) + 7) / 8;
    return passes & 1;
}

// The four raster layouts end on an unpadded last piece plus 256 bytes of slack, and tolerate a base that is not 256-byte
// aligned (the carver rounds it up into that slack).
size_t geom_layout(int P, char* base, GeomView* v) {
    Carver c(base);
    const size_t n = (size_t)(P > 0 ? P : 1);
    GeomView g;
    g.rec = c.take<GaussRec>(n);
    g.cov3D = c.take<float>(6 * n);
    g.tiles_touched = c.take<uint32_t>(n);
    g.clamped = c.take<uint8_t>(n);
    g.sort_keys[0] = c.take<uint32_t>(n);
    g.sort_keys[1] = c.take<uint32_t>(n);
    g.sort_vals[0] = c.take<uint32_t>(n);
    g.sort_vals[1] = c.take<uint32_t>(n);
    g.bigq = g.sort_keys[1];  // (the raw depth keys are consumed by the compaction, the sort's result is in buffer 0)
    g.offsets = c.take<uint32_t>(n);
    g.aux = c.take<uint4>(n);
    g.blk_agg = c.take<uint2>((n + PRE_BLOCK - 1) / PRE_BLOCK);
    // (blk_coarse, counters, sort control words: contiguous, ONE memset clears the three)
    g.blk_coarse = c.take<unsigned long long>((((n + PRE_BLOCK - 1) / PRE_BLOCK + COARSE_BLOCKS - 1) / COARSE_BLOCKS) *
                                              (size_t)COARSE_STRIDE);
    g.counters = c.take<uint32_t>(COUNTER_WORDS);  // directly in front of the sort scratch: one memset clears both
    g.scratch_words = sort_scratch_words(n) + scan_scratch_words(n);
    g.scratch = c.take<uint32_t>(g.scratch_words);
    if (v) *v = g;
    return c.end() + 256;
}

size_t image_layout(int W, int H, char* base, ImageView* v) {
    Carver c(base);
    ImageView im;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    im.n_contrib = c.take<uint32_t>((size_t)W * H);
    im.ranges = c.take<uint2>((size_t)gx * gy);
    im.qcost = c.take<uint32_t>((size_t)gx * gy * 4);
    im.qorder = c.take<uint32_t>((size_t)gx * gy * 4 + 8);
    im.qmask0 = c.take<unsigned long long>((size_t)gx * gy * 4);
    if (v) *v = im;
    return c.end() + 256;
}

size_t bwd_scratch_layout(int N, int S, char* base, BwdScratchView* v) {
    Carver c(base);
    const size_t n = (size_t)(N > 0 ? N : 1) * 4;
    BwdScratchView b;
    b.rows = c.take<float>(n * (size_t)bwd_row_floats(S));
    b.flags = c.take<uint8_t>(n);
    b.cap_big = reduce_cap_big(n / 4);
    b.big_ctl = c.take<uint32_t>(8);
    b.big_desc = c.take<uint4>(b.cap_big);
    b.contrib = c.take<uint8_t>(n / 4);  // (last: everything in front stays where it was)
    if (v) *v = b;
    return c.end() + 256;
}

size_t binning_layout(int N, char* base, BinView* v) {
    Carver c(base);
    const size_t n = (size_t)(N > 0 ? N : 1);
    BinView b;
    b.keys[0] = c.take<uint32_t>(n);
    b.keys[1] = c.take<uint32_t>(n);
    b.vals[0] = c.take<uint32_t>(n);
    b.vals[1] = c.take<uint32_t>(n);
    b.scratch_words = sort_scratch_words(n) + 8;
    b.scratch = c.take<uint32_t>(b.scratch_words);
    b.qmask = c.take<unsigned long long>(4 * (n / 64 + 2));
    if (v) *v = b;
    return c.end() + 256;
}

// common.h: the views of a finished frame, for every entry that takes its three workspaces
FrameViews frame_views(int P, int W, int H, int R, const void* geom, const void* image, const void* binning) {
    FrameViews f{};
    // (the views are the forward's, hence writable.  Through a const workspace an entry writes only what the frame keeps for
    // that very entry: im.qorder, the member masks of a reblend.)
    geom_layout(P, static_cast<char*>(const_cast<void*>(geom)), &f.g);
    if (image) image_layout(W, H, static_cast<char*>(const_cast<void*>(image)), &f.im);
    if (binning) {
        binning_layout(R, static_cast<char*>(const_cast<void*>(binning)), &f.bv);
        f.plist = f.bv.vals[tile_sort_result_index(W, H, R)];
    }
    return f;
}

namespace {

// Starts a row backward on a scratch laid out for `cap` instances: the validity bytes of the slots this frame can use and
// big_ctl are cleared by extra workgroups of the quadrant-order launch (count on the device: 4 x num_rendered bytes, not
// 4 x capacity) -- or by memsets where that launch does not exist.  Returns 1 (the quadrant order is used), 0 or -1 (error).
int start_row_backward(const GoiRasterScene& sc, const FrameViews& f, const BwdScratchView& scr, int cap, hipStream_t s) {
    if (launch_quad_order(sc, f.im, s, scr.flags, f.g.counters + COUNTER_N, (uint32_t)cap, scr.big_ctl)) return 1;
    GOI_HIP(hipMemsetAsync(scr.flags, 0, round_up_256((size_t)cap * 4), s));  // (the layout ends with 256 spare bytes)
    GOI_HIP(hipMemsetAsync(scr.big_ctl, 0, 8 * sizeof(uint32_t), s));
    return 0;
}

// the per-tile backward blend accumulates with atomics: its six arrays (P Gaussians, S channels) start from zero
int zero_blend_grads(const BlendGrads& b, size_t P, int S, hipStream_t s) {
    GOI_HIP(hipMemsetAsync(b.dL_dmean2D, 0, 3 * P * sizeof(float), s));
    GOI_HIP(hipMemsetAsync(b.dL_dconic, 0, 4 * P * sizeof(float), s));
    GOI_HIP(hipMemsetAsync(b.dL_dopacity, 0, P * sizeof(float), s));
    GOI_HIP(hipMemsetAsync(b.dL_dcolor, 0, 3 * P * sizeof(float), s));
    GOI_HIP(hipMemsetAsync(b.dL_dsemantic, 0, (size_t)S * P * sizeof(float), s));
    GOI_HIP(hipMemsetAsync(b.dL_ddepth, 0, P * sizeof(float), s));
    return 0;
}

// the form of the row blend kernels the process-wide switches ask for (launch_render_bwd_rows / _sem)
bool option_exact_flush() { return (g_options.bwd_variant & 15) == 2; }
bool option_walk_masks() { return g_options.bwd_masks != 0; }

}  // namespace

}  // namespace goi

using namespace goi;

extern "C" {

int goi_raster_abi_version(void) { return GOI_RASTER_ABI_VERSION; }
const char* goi_raster_last_error(void) { return g_err.c_str(); }

// Sizes are computed with a base that already has the strictest alignment, so they are upper
// bounds for any 256-byte aligned buffer; +256 slack covers callers that hand over less.
size_t goi_raster_geom_bytes(int P) { return geom_layout(P, nullptr, nullptr) + 256; }
size_t goi_raster_image_bytes(int W, int H) { return image_layout(W, H, nullptr, nullptr) + 256; }
size_t goi_raster_binning_bytes(int N) { return binning_layout(N, nullptr, nullptr) + 256; }
size_t goi_raster_backward_scratch_bytes(int N, int S) { return bwd_scratch_layout(N, S, nullptr, nullptr) + 256; }
size_t goi_raster_debug_backward_contrib_offset(int N, int S) {
    BwdScratchView v;
    char* const base = reinterpret_cast<char*>(256);  // (never dereferenced: the carver hands out no pointers from NULL)
    bwd_scratch_layout(N, S, base, &v);
    return (size_t)(reinterpret_cast<char*>(v.contrib) - base);  // the offset in a 256-byte aligned scratch
}

// keep (or NULL) / invert: the per-Gaussian selection
int goi_raster_forward(const GoiRasterScene* scene, void* geom_buffer, void* image_buffer, goi_alloc_fn binning_alloc,
                       void* alloc_user, float* out_color, float* out_semantic, float* out_depth, float* out_alpha,
                       int* radii, const uint8_t* keep, int invert, void* stream) {
    refresh_options();
    if (validate(scene, true)) return -1;
    const GoiRasterScene& sc = *scene;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t HW = (size_t)sc.W * sc.H;
    if (sc.P == 0) {  // zero-filled outputs, nothing launched (DGR/rasterize_points.cu:84-85)
        GOI_HIP(hipMemsetAsync(out_color, 0, 3 * HW * sizeof(float), s));
        GOI_HIP(hipMemsetAsync(out_semantic, 0, (size_t)sc.S * HW * sizeof(float), s));
        GOI_HIP(hipMemsetAsync(out_depth, 0, HW * sizeof(float), s));
        GOI_HIP(hipMemsetAsync(out_alpha, 0, HW * sizeof(float), s));
        return 0;
    }
    if (!geom_buffer || !image_buffer || !binning_alloc) return fail("workspace pointer / allocator is NULL");
    GeomView g;
    ImageView im;
    geom_layout(sc.P, static_cast<char*>(geom_buffer), &g);
    image_layout(sc.W, sc.H, static_cast<char*>(image_buffer), &im);
    const uint32_t* plist = nullptr;
    unsigned long long* qmask = nullptr;
    const int N = geometry_and_binning(sc, g, im, binning_alloc, alloc_user, radii, &plist, s, &qmask, keep, invert);
    if (N < 0) return -1;
    {
        StageTimer t(GOI_STAGE_BLEND_FWD, s);
        launch_render_fwd(sc, g, im, plist, out_color, out_semantic, out_depth, out_alpha, s, qmask);
    }
    if (check_stage(sc, s, "forward blend")) return -1;
    GOI_HIP(hipGetLastError());
    return N;
}

int goi_raster_forward_async(const GoiRasterScene* scene, void* geom_buffer, void* image_buffer, void* binning_buffer,
                             int capacity, float* out_color, float* out_semantic, float* out_depth, float* out_alpha,
                             int* radii, const float* zcut_in, float* zcut_out, const uint8_t* keep, int invert, void* stream) {
    refresh_options();
    if (validate(scene, true)) return -1;
    const GoiRasterScene& sc = *scene;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (sc.P == 0) return fail("goi_raster_forward_async: P == 0 has nothing to speculate on; use goi_raster_forward");
    if (sc.debug) return fail("goi_raster_forward_async: debug mode synchronises after every stage; use goi_raster_forward");
    if (g_options.sort_variant != 1) return fail("goi_raster_forward_async needs the onesweep sort (sort_variant 1)");
    if (capacity <= 0) return fail("goi_raster_forward_async: capacity must be positive");
    if (!geom_buffer || !image_buffer || !binning_buffer) return fail("workspace pointer is NULL");
    if (keep && (zcut_in || zcut_out)) return fail("goi_raster_forward_async: a selection (keep) cannot be combined with a depth cut");
    GeomView g;
    ImageView im;
    BinView bv;
    geom_layout(sc.P, static_cast<char*>(geom_buffer), &g);
    image_layout(sc.W, sc.H, static_cast<char*>(image_buffer), &im);
    binning_layout(capacity, static_cast<char*>(binning_buffer), &bv);
    const int ticket = ticket_acquire(capacity);
    if (ticket < 0) return -1;
    const uint32_t* order = nullptr;
    const uint32_t* plist = nullptr;
    uint32_t* zlearn = reinterpret_cast<uint32_t*>(zcut_out);  // (positive floats: the kernels take their maximum as integers)
    if (enqueue_front(sc, g, im, radii, /*ticket=*/-1, &order, s, zcut_in, zlearn, keep, invert) ||
        enqueue_back(sc, g, im, bv, capacity, /*exact=*/false, order, radii, &plist, s)) {
        ticket_release(ticket);
        return -1;
    }
    // The frame's counters reach the host without a copy of their own: a wave of the forward blend stores the 32 head words
    // into the ticket's pinned (device-mapped) words and then, behind a system-scope fence, the ticket's sequence number
    // (STAMP_WORD): the ticket resolves when that wave has run -- i.e. when the blend has STARTED, not when the frame's kernels
    // have finished (the counters are final before the blend starts; a caller that needs the images synchronises the stream as
    // for any other kernel).  The runtime moved a 128-byte device-to-host copy as two copy kernels per frame, and an event behind
    // the blend cost the stream a bubble.  A frame whose lists were CUT, or that learns a cut, may still raise
    // its flag inside the blend (the cut is checked there, whether or not zcut_out was given), so it keeps the copy behind the
    // kernel: the words a blend wave stores are a snapshot taken when the kernel STARTS.
    uint32_t* host_words = nullptr;
    uint32_t stamp = 0;
    {
        std::lock_guard<std::mutex> lk(g_ticket_mu);
        Ticket& tk = g_tickets[ticket];
        if (!zlearn && !zcut_in && tk.pinned_dev) {
            host_words = tk.pinned_dev;
            tk.seq = tk.seq + 1u ? tk.seq + 1u : 1u;  // (never 0: a fresh ticket's stamp word)
            stamp = tk.seq;
            tk.head_only = true;
            tk.stamped = true;  // no copy, no event: ticket_result compares pinned[STAMP_WORD] with seq
            tk.stream = s;
        }
    }
    {
        StageTimer t(GOI_STAGE_BLEND_FWD, s);
        launch_render_fwd(sc, g, im, plist, out_color, out_semantic, out_depth, out_alpha, s, bv.qmask, zcut_in, zlearn,
                          host_words, stamp);
    }
    if (host_words) {
    } else if (enqueue_readback(g, ticket, s, /*head_only=*/true)) {
        ticket_release(ticket);
        return -1;
    }
    if (hipGetLastError() != hipSuccess) {
        ticket_release(ticket);
        return fail("goi_raster_forward_async: a launch failed");
    }
    return ticket;
}

int goi_raster_ticket_result(int ticket, int wait, int* num_rendered, unsigned* frame_flags) {
    long long n = 0;
    unsigned fl = 0;
    const int r = ticket_result(ticket, wait, &n, &fl);
    if (r == 1 && num_rendered) *num_rendered = (int)n;
    if (r == 1 && frame_flags) *frame_flags = fl;
    return r;
}

int goi_raster_forward_redo(const GoiRasterScene* scene, int num_rendered, void* geom_buffer, void* image_buffer,
                            void* binning_buffer, float* out_color, float* out_semantic, float* out_depth,
                            float* out_alpha, const int* radii, void* stream) {
    refresh_options();
    // (the back half of a frame reads P, S, W, H, the semantic rows and the background from the scene; everything else
    // comes from the geometry workspace of the first attempt, so only those fields are checked)
    if (!scene) return fail("scene is NULL");
    const GoiRasterScene& sc = *scene;
    if (sc.P <= 0 || sc.W <= 0 || sc.H <= 0 || sc.S < 1 || sc.S > 32) return fail("goi_raster_forward_redo: bad P/W/H/S");
    if (!sc.semantics || !sc.bg || !radii) return fail("goi_raster_forward_redo: semantics, bg and radii are required");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_rendered < 0) return fail("goi_raster_forward_redo: nothing to redo");
    if (!geom_buffer || !image_buffer || (num_rendered > 0 && !binning_buffer)) return fail("workspace pointer is NULL");
    GeomView g;
    ImageView im;
    BinView bv;
    geom_layout(sc.P, static_cast<char*>(geom_buffer), &g);
    image_layout(sc.W, sc.H, static_cast<char*>(image_buffer), &im);
    binning_layout(num_rendered, static_cast<char*>(binning_buffer), &bv);
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    // the geometry state of the first attempt (records, depth order, offsets) does not depend on the capacity and is
    // still in the geometry buffer; the per-tile counts the first emit accumulated are not wanted
    GOI_HIP(hipMemsetAsync(im.ranges, 0, sizeof(uint2) * (size_t)gx * gy, s));
    const uint32_t* order = g.sort_vals[depth_sort_result_index()];
    const uint32_t* plist = nullptr;
    if (enqueue_back(sc, g, im, bv, num_rendered, /*exact=*/true, order, radii, &plist, s)) return -1;
    {
        StageTimer t(GOI_STAGE_BLEND_FWD, s);
        launch_render_fwd(sc, g, im, plist, out_color, out_semantic, out_depth, out_alpha, s, bv.qmask);
    }
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_forward_reblend(const GoiRasterScene* scene, int R, const void* geom_buffer, const void* binning_buffer,
                               const void* cached_image_buffer, void* image_buffer, float* out_color, float* out_semantic,
                               float* out_depth, float* out_alpha, void* stream) {
    refresh_options();
    // (only the blend runs: it reads P, S, W, H, the semantic rows and the background from the scene; the Gaussian records,
    // the tile lists and the tile ranges are those of the frame that filled the workspaces)
    if (!scene) return fail("scene is NULL");
    const GoiRasterScene& sc = *scene;
    if (sc.P <= 0 || sc.W <= 0 || sc.H <= 0 || sc.S < 1 || sc.S > 32) return fail("goi_raster_forward_reblend: bad P/W/H/S");
    if (!sc.semantics || !sc.bg) return fail("goi_raster_forward_reblend: semantics and bg are required");
    if (R < 0) return fail("goi_raster_forward_reblend: bad R");
    if (!geom_buffer || !cached_image_buffer || !image_buffer || (R > 0 && !binning_buffer))
        return fail("workspace pointer is NULL");
    if (!out_color || !out_semantic || !out_depth || !out_alpha) return fail("output pointer is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FrameViews f = frame_views(sc.P, sc.W, sc.H, R, geom_buffer, cached_image_buffer, binning_buffer);
    ImageView im;
    image_layout(sc.W, sc.H, static_cast<char*>(image_buffer), &im);
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    // the new frame gets its own image state (n_contrib is written by the blend and read by ITS backward); the tile ranges
    // are the cached frame's
    GOI_HIP(hipMemcpyAsync(im.ranges, f.im.ranges, sizeof(uint2) * (size_t)gx * gy, hipMemcpyDeviceToDevice, s));
    {
        // (the member masks of rounds >= 1 go into the CACHED binning workspace: they depend on geometry and tile lists only,
        // so every reblend of this camera writes the words that are already there)
        StageTimer t(GOI_STAGE_BLEND_FWD, s);
        launch_render_fwd(sc, f.g, im, f.plist, out_color, out_semantic, out_depth, out_alpha, s, f.bv.qmask);
    }
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_trace(const GoiRasterScene* scene, const float* img_sem, void* geom_buffer, void* image_buffer,
                     goi_alloc_fn binning_alloc, void* alloc_user, float* out_color, float* gau_sem, int* num_gsem,
                     int* radii, void* stream) {
    refresh_options();
    if (validate(scene, false)) return -1;
    const GoiRasterScene& sc = *scene;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t HW = (size_t)sc.W * sc.H;
    GOI_HIP(hipMemsetAsync(out_color, 0, 3 * HW * sizeof(float), s));
    if (sc.P == 0) return 0;
    if (!img_sem) return fail("img_sem is NULL");
    if (!geom_buffer || !image_buffer || !binning_alloc) return fail("workspace pointer / allocator is NULL");
    GOI_HIP(hipMemsetAsync(gau_sem, 0, (size_t)sc.P * sc.S * sizeof(float), s));
    GOI_HIP(hipMemsetAsync(num_gsem, 0, (size_t)sc.P * sizeof(int), s));
    GeomView g;
    ImageView im;
    geom_layout(sc.P, static_cast<char*>(geom_buffer), &g);
    image_layout(sc.W, sc.H, static_cast<char*>(image_buffer), &im);
    const uint32_t* plist = nullptr;
    const int N = geometry_and_binning(sc, g, im, binning_alloc, alloc_user, radii, &plist, s);
    if (N < 0) return -1;
    launch_trace_fwd(sc, img_sem, g, im, plist, out_color, gau_sem, num_gsem, s);
    if (check_stage(sc, s, "trace")) return -1;
    GOI_HIP(hipGetLastError());
    return N;
}

int goi_raster_backward(const GoiRasterScene* scene, int R, int scratch_instances, int flags, const void* geom_buffer,
                        const void* binning_buffer, const void* image_buffer, const int* radii, const float* out_alpha,
                        const float* dL_dout_color, const float* dL_dout_semantic, const float* dL_dout_depth,
                        const float* dL_dout_alpha, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                        float* dL_dsemantic, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                        float* dL_dscale, float* dL_drot, void* scratch, const int* prev_radii, const uint8_t* prev_mask,
                        uint8_t* row_mask, void* stream) {
    refresh_options();
    if (validate(scene, true, false)) return -1;  // opacity lives in the forward's records
    const GoiRasterScene& sc = *scene;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t P = (size_t)sc.P;
    if (P == 0) return 0;
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail("workspace pointer is NULL");
    const FrameViews f = frame_views(sc.P, sc.W, sc.H, R, geom_buffer, image_buffer, binning_buffer);
    const PixelGrads dpix{dL_dout_color, dL_dout_semantic, dL_dout_depth, dL_dout_alpha};
    const BlendGrads blend{dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dsemantic, dL_ddepth};
    // what every branch below hands to the per-Gaussian backward; a branch adds its own source of the blend gradients
    PreprocessBwdArgs pa;
    pa.blend = blend;
    pa.out = GaussGrads{dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot};
    pa.row_mask = row_mask;
    const bool rows_path = scratch != nullptr && (g_options.bwd_variant & 15) != 1;
    if (scratch_instances < 0 || scratch_instances > R) return fail("scratch_instances must be in 0..R (0: the scratch is laid out for R)");
    // Rs: instances the ROW SCRATCH holds rows for (the binning workspace keeps R); every slot index is below 4 x num_rendered <= 4 Rs
    const int Rs = scratch_instances > 0 ? scratch_instances : R;
    const bool accumulate = (flags & GOI_BACKWARD_ACCUMULATE) != 0;
    if (accumulate && (!rows_path || g_options.bwd_records != 1 || prev_radii || (sc.shs && !dL_dsh) || sc.debug))
        return fail("GOI_BACKWARD_ACCUMULATE needs the default backward (scratch given, bwd_variant 0 / 2, bwd_records 1), dL_dsh when "
                    "the colours are SH, prev_radii NULL and debug off");
    if (accumulate && (prev_mask || row_mask)) return fail("GOI_BACKWARD_ACCUMULATE: prev_mask and row_mask must be NULL");
    if (rows_path) {
        // atomic-free path: (quadrant, Gaussian) partial rows + validity bytes, then a fixed-order sum
        BwdScratchView scr;
        bwd_scratch_layout(Rs, sc.S, static_cast<char*>(scratch), &scr);
        {
            StageTimer t(GOI_STAGE_BLEND_BWD, s);
            if (R > 0) {
                if (start_row_backward(sc, f, scr, Rs, s) < 0) return -1;
                launch_render_bwd_rows(sc, f.g, f.im, f.plist, radii, out_alpha, dpix, scr, option_exact_flush(),
                                       option_walk_masks(), s, f.bv.qmask);
            }
        }
        if (check_stage(sc, s, "backward blend")) return -1;
        StageTimer t(GOI_STAGE_PREPROCESS_BWD, s);
        if (g_options.bwd_records) {  // the blend gradients stay in the row scratch; the kernel skips rows that hold zeros already
            pa.rows = scr.rows;
            pa.prev_radii = prev_radii;
            pa.prev_mask = prev_mask;
        }
        if (g_options.bwd_records == 2 && bwd_row_floats(sc.S) == 32 && R > 0 && !accumulate) {
            // the per-Gaussian backward sums its Gaussians' rows itself; only the BIG Gaussians pass through reduce_big_k's records
            launch_reduce_big_only(sc, f.g, Rs, scr, s);
            pa.flags = scr.flags;
            pa.n_cap = Rs;
        } else if (g_options.bwd_records) {
            // the sums stay in the row scratch (one record per listed Gaussian); preprocess_bwd_k writes the per-id outputs.
            // bwd_skip_idle: the reduction publishes a contribution byte per listed Gaussian and stores no all-zero record;
            // preprocess_bwd_k runs its chain only for the Gaussians that reached a pixel
            uint8_t* contrib = g_options.bwd_skip_idle ? scr.contrib : nullptr;
            launch_reduce_rows(sc, f.g, Rs, scr, BlendGrads{}, s, true, contrib);
            pa.contrib = contrib;
            pa.accumulate = accumulate;
        } else {
            // (every row is written: the previous mask is not consulted, this frame's is still produced)
            launch_reduce_rows(sc, f.g, Rs, scr, blend, s);
        }
        launch_preprocess_bwd(sc, f.g, radii, pa, s);
    } else {
        // atomic path
        if (zero_blend_grads(blend, P, sc.S, s) < 0) return -1;
        if (R > 0) {
            StageTimer t(GOI_STAGE_BLEND_BWD, s);
            launch_render_bwd_tile(sc, f.g, f.im, f.plist, out_alpha, dpix, blend, s);
        }
        if (check_stage(sc, s, "backward blend")) return -1;
        StageTimer t(GOI_STAGE_PREPROCESS_BWD, s);
        launch_preprocess_bwd(sc, f.g, radii, pa, s);
    }
    if (check_stage(sc, s, "backward preprocess")) return -1;
    GOI_HIP(hipGetLastError());
    return 0;
}

int goi_raster_backward_semantics(const GoiRasterScene* scene, int R, const void* geom_buffer, const void* binning_buffer,
                                  const void* image_buffer, const int* radii, const float* out_alpha,
                                  const float* dL_dout_semantic, float* dL_dsemantic, void* scratch, void* stream) {
    refresh_options();
    if (validate(scene, true, false)) return -1;
    const GoiRasterScene& sc = *scene;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (sc.P == 0) return 0;
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail("workspace pointer is NULL");
    if (!scratch) return fail("goi_raster_backward_semantics needs the scratch of goi_raster_backward_scratch_bytes");
    if (!dL_dout_semantic || !dL_dsemantic || !out_alpha || !radii) return fail("a required pointer is NULL");
    const FrameViews f = frame_views(sc.P, sc.W, sc.H, R, geom_buffer, image_buffer, binning_buffer);
    BwdScratchView scr;  // same allocation as the full backward; rows are narrower here
    bwd_scratch_layout(R, sc.S, static_cast<char*>(scratch), &scr);
    const int row_floats = bwd_sem_row_floats(sc.S);
    {
        StageTimer t(GOI_STAGE_BLEND_BWD, s);
        if (R > 0) {
            if (start_row_backward(sc, f, scr, R, s) < 0) return -1;
            launch_render_bwd_sem(sc, f.g, f.im, f.plist, radii, out_alpha, dL_dout_semantic, scr.rows, scr.flags, row_floats,
                                  option_exact_flush(), option_walk_masks(), s, f.bv.qmask);
        }
    }
    if (check_stage(sc, s, "backward blend (semantics)")) return -1;
    StageTimer t(GOI_STAGE_PREPROCESS_BWD, s);
    launch_reduce_sem_rows(sc, f.g, R, scr, row_floats, dL_dsemantic, s);
    GOI_HIP(hipGetLastError());
    return 0;
}

const uint32_t* goi_raster_truncated_flag(const void* geom_buffer, int P) {
    if (!geom_buffer || P <= 0) return nullptr;
    return frame_views(P, 0, 0, 0, geom_buffer, nullptr, nullptr).g.counters + COUNTER_OVF;
}

void goi_raster_profile_enable(int on) { g_profile_mask.store(on ? ~0u : 0u); }

void goi_raster_profile_stages(unsigned stage_mask) { g_profile_mask.store(stage_mask); }

int goi_raster_set_option(const char* name, int value) {
    if (!name) return fail("option name is NULL");
    std::lock_guard<std::mutex> lk(g_options_mu);
    Options& g_options = g_shared_options;  // (calls already running keep their own snapshot)
    if (!strcmp(name, "fwd_variant")) {
        if (value < 0 || value > 1) return fail("fwd_variant must be 0 or 1");
        g_options.fwd_variant = value;
    }
    else if (!strcmp(name, "bwd_variant")) {
        if (value < 0 || value > 2) return fail("bwd_variant must be 0, 1 or 2");
        g_options.bwd_variant = value;
    }
    else if (!strcmp(name, "sort_variant")) g_options.sort_variant = value;
    else if (!strcmp(name, "sort_small")) g_options.sort_small = value;
    else if (!strcmp(name, "sort_lookback")) g_options.sort_lookback = value;
    else if (!strcmp(name, "cull_variant")) g_options.cull_variant = value;
    else if (!strcmp(name, "bwd_order")) {
        if (value < 0 || value > 8) return fail("bwd_order must be 0 .. 8");
        g_options.bwd_order = value;
    }
    else if (!strcmp(name, "decode_variant")) g_options.decode_variant = value;
    else if (!strcmp(name, "bwd_masks")) {
        if (value < 0 || value > 1) return fail("bwd_masks must be 0 or 1");
        g_options.bwd_masks = value;
    }
    else if (!strcmp(name, "bwd_records")) {
        if (value < 0 || value > 2) return fail("bwd_records must be 0, 1 or 2");
        g_options.bwd_records = value;
    }
    else if (!strcmp(name, "bwd_skip_idle")) {
        if (value < 0 || value > 1) return fail("bwd_skip_idle must be 0 or 1");
        g_options.bwd_skip_idle = value;
    }
    else if (!strcmp(name, "osh_path")) {
        if (value < 0 || value > 1) return fail("osh_path must be 0 or 1");
        g_options.osh_path = value;
    }
    else return fail(std::string("unknown option ") + name);
    return 0;
}

int goi_raster_profile_collect(double* ms, int* calls) {
    std::vector<StageEvents> events;
    {
        std::lock_guard<std::mutex> lk(g_profile_mu);
        events.swap(g_events);
    }
    for (auto& ev : events) {
        GOI_HIP(hipEventSynchronize(ev.b));
        float t = 0.f;
        GOI_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
        if (ms) ms[ev.stage] += (double)t;
        if (calls) calls[ev.stage] += 1;
        std::lock_guard<std::mutex> lk(g_profile_mu);
        g_pool.push_back(ev.a);
        g_pool.push_back(ev.b);
    }
    return 0;
}

int goi_raster_debug_views(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                           const void* image_buffer, float* depths, float* means2D, float* conic_opacity, float* rgb,
                           uint32_t* tiles_touched, uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib,
                           void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P <= 0) return 0;
    const FrameViews f = frame_views(P, W, H, R, geom_buffer, image_buffer, binning_buffer);
    const GeomView& g = f.g;
    const ImageView& im = f.im;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    // strided copies out of the 48-byte records
    const char* rec = reinterpret_cast<const char*>(g.rec);
    const size_t pitch = sizeof(GaussRec);
    if (means2D) GOI_HIP(hipMemcpy2DAsync(means2D, 8, rec + 0, pitch, 8, P, hipMemcpyDeviceToDevice, s));
    if (conic_opacity) {  // (a,b) then (c,o)
        GOI_HIP(hipMemcpy2DAsync(conic_opacity, 16, rec + 8, pitch, 8, P, hipMemcpyDeviceToDevice, s));
        GOI_HIP(hipMemcpy2DAsync(reinterpret_cast<char*>(conic_opacity) + 8, 16, rec + 16, pitch, 8, P,
                                 hipMemcpyDeviceToDevice, s));
    }
    if (depths) GOI_HIP(hipMemcpy2DAsync(depths, 4, rec + 44, pitch, 4, P, hipMemcpyDeviceToDevice, s));
    if (rgb) GOI_HIP(hipMemcpy2DAsync(rgb, 12, rec + 32, pitch, 12, P, hipMemcpyDeviceToDevice, s));
    if (tiles_touched)
        GOI_HIP(hipMemcpyAsync(tiles_touched, g.tiles_touched, sizeof(uint32_t) * P, hipMemcpyDeviceToDevice, s));
    if (ranges) GOI_HIP(hipMemcpyAsync(ranges, im.ranges, sizeof(uint2) * gx * gy, hipMemcpyDeviceToDevice, s));
    if (n_contrib)
        GOI_HIP(hipMemcpyAsync(n_contrib, im.n_contrib, sizeof(uint32_t) * (size_t)W * H, hipMemcpyDeviceToDevice, s));
    if (point_list && R > 0)
        GOI_HIP(hipMemcpyAsync(point_list, f.plist, sizeof(uint32_t) * (size_t)R, hipMemcpyDeviceToDevice, s));
    return 0;
}

int goi_raster_debug_backward_blend(const GoiRasterScene* scene, int R, int mode, const void* geom_buffer,
                                    const void* binning_buffer, const void* image_buffer, const int* radii,
                                    const float* out_alpha, const float* dL_dout_color, const float* dL_dout_semantic,
                                    const float* dL_dout_depth, const float* dL_dout_alpha, void* scratch, float* rows,
                                    uint8_t* row_flags, uint32_t* aux, unsigned long long* qmask0, unsigned long long* qmask,
                                    uint32_t* qcost, uint32_t* qorder, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                    float* dL_dcolor, float* dL_dsemantic, float* dL_ddepth, void* stream) {
    const std::string fn = "goi_raster_debug_backward_blend";
    refresh_options();
    if (!scene) return fail(fn + ": scene is NULL");
    const GoiRasterScene& sc = *scene;
    if (sc.P <= 0 || sc.W <= 0 || sc.H <= 0) return fail(fn + ": bad P/W/H");
    if (sc.S < 1 || sc.S > 32) return fail(fn + ": need 1 <= S <= 32");
    if (R <= 0) return fail(fn + ": need R > 0 (the instance count the forward returned)");
    if (mode < 0 || mode > 8)
        return fail(fn + ": unknown mode (0..3 rows, 4..7 semantic rows: bit 0 exact-fp32 flush, bit 1 candidate testing; 8 per-tile kernel)");
    const bool tile = mode == 8, sem = !tile && (mode & 4) != 0;
    if (!sc.bg || !sc.semantics) return fail(fn + ": scene.bg and scene.semantics are required");
    if ((sc.S & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.semantics) & 15u) != 0)
        return fail(fn + ": semantics must be 16-byte aligned when S is a multiple of 4");
    if (!geom_buffer || !binning_buffer || !image_buffer) return fail(fn + ": workspace pointer is NULL");
    if (check_workspace(fn, geom_buffer, "geom_buffer") < 0 || check_workspace(fn, binning_buffer, "binning_buffer") < 0 ||
        check_workspace(fn, image_buffer, "image_buffer") < 0)
        return -1;
    if (!radii || !out_alpha) return fail(fn + ": radii and out_alpha are required");
    if (sem && !dL_dout_semantic) return fail(fn + ": the semantic rows need dL_dout_semantic");
    if (tile) {
        if (!dL_dmean2D || !dL_dconic || !dL_dopacity || !dL_dcolor || !dL_dsemantic || !dL_ddepth)
            return fail(fn + ": mode 8 writes the six per-id arrays");
    } else {
        if (!scratch) return fail(fn + ": modes 0..7 need the scratch of goi_raster_backward_scratch_bytes");
        if (check_workspace(fn, scratch, "scratch") < 0) return -1;
        if (!rows || !row_flags) return fail(fn + ": modes 0..7 copy out rows and row_flags");
        if (reinterpret_cast<uintptr_t>(rows) & 15u) return fail(fn + ": rows must be 16-byte aligned");
    }
    if ((aux && (reinterpret_cast<uintptr_t>(aux) & 15u)) || (qmask0 && (reinterpret_cast<uintptr_t>(qmask0) & 7u)) ||
        (qmask && (reinterpret_cast<uintptr_t>(qmask) & 7u)))
        return fail(fn + ": aux must be 16-byte aligned, qmask0 and qmask 8-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const FrameViews f = frame_views(sc.P, sc.W, sc.H, R, geom_buffer, image_buffer, binning_buffer);
    const PixelGrads dpix{dL_dout_color, dL_dout_semantic, dL_dout_depth, dL_dout_alpha};
    const int gx = (sc.W + TILE - 1) / TILE, gy = (sc.H + TILE - 1) / TILE;
    const size_t n_quads = (size_t)gx * gy * 4;
    int ordered = 0;
    if (tile) {
        const BlendGrads blend{dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dsemantic, dL_ddepth};
        if (zero_blend_grads(blend, (size_t)sc.P, sc.S, s) < 0) return -1;
        launch_render_bwd_tile(sc, f.g, f.im, f.plist, out_alpha, dpix, blend, s);
    } else {
        // the form of the kernel is the mode's, whatever the process-wide switches say
        const bool exact_flush = (mode & 1) != 0, walk_masks = (mode & 2) == 0;
        BwdScratchView scr;
        bwd_scratch_layout(R, sc.S, static_cast<char*>(scratch), &scr);
        ordered = start_row_backward(sc, f, scr, R, s);
        if (ordered < 0) return -1;
        const int row_floats = sem ? bwd_sem_row_floats(sc.S) : bwd_row_floats(sc.S);
        if (sem)
            launch_render_bwd_sem(sc, f.g, f.im, f.plist, radii, out_alpha, dL_dout_semantic, scr.rows, scr.flags, row_floats,
                                  exact_flush, walk_masks, s, f.bv.qmask);
        else
            launch_render_bwd_rows(sc, f.g, f.im, f.plist, radii, out_alpha, dpix, scr, exact_flush, walk_masks, s, f.bv.qmask);
        GOI_HIP(hipGetLastError());
        GOI_HIP(hipMemcpyAsync(rows, scr.rows, (size_t)R * 4 * row_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        GOI_HIP(hipMemcpyAsync(row_flags, scr.flags, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    }
    GOI_HIP(hipGetLastError());
    if (aux) GOI_HIP(hipMemcpyAsync(aux, f.g.aux, (size_t)sc.P * sizeof(uint4), hipMemcpyDeviceToDevice, s));
    if (qmask0) GOI_HIP(hipMemcpyAsync(qmask0, f.im.qmask0, n_quads * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    if (qmask)
        GOI_HIP(hipMemcpyAsync(qmask, f.bv.qmask, 4 * ((size_t)R / 64 + 2) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    if (qcost) GOI_HIP(hipMemcpyAsync(qcost, f.im.qcost, n_quads * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (qorder && ordered)
        GOI_HIP(hipMemcpyAsync(qorder, f.im.qorder, 8 * ((n_quads + 7) / 8) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return ordered;
}

}  // extern "C"
