// mdt_handle.h -- host-side bookkeeping shared by the three stateful handles: the denoiser (mdt_model.hip, mdt_train.hip),
// the Perceiver resampler (mdt_resampler.hip) and the MAP pooling head (mdt_map_pool.hip).  Parameter slots and their
// upload, the pool of training tapes with its release guard across streams, and the batch-sized device blocks that grow
// on demand (workspace, tapes, backward scratch).  Each module keeps its own parameter layout and gradient layout rule.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "mdt_internal.h"

// ------------------------------------------------------------------------------------------------
// parameter slots
// ------------------------------------------------------------------------------------------------
// TRANSPOSE: (rows, K) -> (K, rows);  PAD_COLS: (rows, K) -> (rows, n_off) row-major, columns K.. stay zero
enum SlotKind { SLOT_PACK = 0, SLOT_RAW = 1, SLOT_TRANSPOSE = 2, SLOT_PAD_COLS = 3, SLOT_PACK_T = 4,  // PACK_T: fragment image of the TRANSPOSE of a (rows, K) matrix
                SLOT_PACK_SPLIT = 5 };  // three-way bf16 split fragment image of a (rows, K) matrix (mdt_mlp_split.h): 6 rows K bytes at dst

struct Slot {
    std::string name;
    int64_t numel = 0;
    int kind = SLOT_RAW;
    float* dst = nullptr;  // packed image base (SLOT_PACK) or raw destination (SLOT_RAW)
    int rows = 0, K = 0, n_off = 0;
    bool loaded = false;
    Lin* lin = nullptr;    // SLOT_PACK: the Linear this part belongs to (training keeps a transposed image too)
};

static inline Slot* mdt_find_slot(std::vector<Slot>& slots, const std::string& name) {
    for (Slot& c : slots)
        if (c.name == name) return &c;
    return nullptr;
}

// fn: the entry point named in the message
static inline mdt_status mdt_check_numel(const char* fn, const char* name, int64_t numel, const Slot& slot) {
    if (numel == slot.numel) return MDT_OK;
    return mdt_fail(MDT_ERR_INVALID_ARG, "%s: '%s' has %lld elements, expected %lld", fn, name, (long long)numel,
                    (long long)slot.numel);
}

// *dev = the device image of a parameter source: src itself in device memory, else its copy in `staging` (made once: a
// non-null *dev is kept)
static inline mdt_status mdt_stage_source(const float* src, int64_t numel, float* staging, hipStream_t s, const float** dev) {
    if (*dev) return MDT_OK;
    hipPointerAttribute_t attr;
    hipError_t pe = hipPointerGetAttributes(&attr, src);
    if (pe == hipSuccess && attr.type == hipMemoryTypeDevice) {
        *dev = src;
    } else {
        (void)hipGetLastError();  // unregistered host memory reports an error: clear it
        HIP_TRY(hipMemcpyAsync(staging, src, numel * sizeof(float), hipMemcpyHostToDevice, s));
        *dev = staging;
    }
    return MDT_OK;
}

// one parameter (a (rows, K) row-major source in host or device memory) into one slot of kind RAW / PAD_COLS / TRANSPOSE /
// PACK_T / PACK; *dev caches the staged source across the slots of one load (nullptr before the first)
static inline mdt_status mdt_upload_slot(const Slot& t, const float* src, int64_t numel, float* staging, hipStream_t s,
                                         const float** dev) {
    if (t.kind == SLOT_RAW) {
        HIP_TRY(hipMemcpyAsync(t.dst, src, numel * sizeof(float), hipMemcpyDefault, s));
        return MDT_OK;
    }
    if (t.kind == SLOT_PAD_COLS) {  // (rows, K) -> (rows, n_off): the pad columns keep the arena's zeros
        HIP_TRY(hipMemcpy2DAsync(t.dst, (size_t)t.n_off * sizeof(float), src, (size_t)t.K * sizeof(float),
                                 (size_t)t.K * sizeof(float), (size_t)t.rows, hipMemcpyDefault, s));
        return MDT_OK;
    }
    MDT_TRY(mdt_stage_source(src, numel, staging, s, dev));
    if (t.kind == SLOT_TRANSPOSE) HIP_TRY(mdt_launch_transpose(*dev, t.dst, t.rows, t.K, s));
    else if (t.kind == SLOT_PACK_T) HIP_TRY(mdt_launch_pack_weight_t(*dev, t.rows, t.K, t.K, t.dst, 0, t.rows / 16, s));  // image of the transpose
    else HIP_TRY(mdt_launch_pack_weight(*dev, t.rows, t.K, t.dst, t.n_off, s));
    if (t.kind == SLOT_PACK && t.lin && t.lin->wt)  // training: image of W^T for dX = dY W
        HIP_TRY(mdt_launch_pack_weight_t(*dev, t.rows, t.K, t.K, t.lin->wt, t.n_off, t.lin->N / 16, s));
    return MDT_OK;
}

// "<what> '<name>' <when>" for the first slot that holds no upload
static inline mdt_status mdt_check_loaded(const std::vector<Slot>& slots, const char* what, const char* when = "was never loaded") {
    for (const Slot& s : slots)
        if (!s.loaded) return mdt_fail(MDT_ERR_NOT_LOADED, "%s '%s' %s", what, s.name.c_str(), when);
    return MDT_OK;
}

// the parameters of a single-target module (resampler, MAP pool): one arena of images, the upload staging buffer and, once
// training is prepared, the W^T images and the per-slot offsets of the flat gradient (laid out by the module)
struct ParamTable {
    float* arena = nullptr;
    std::vector<Slot> slots;
    float* staging = nullptr;
    float* wt_arena = nullptr;
    std::vector<int64_t> grad_off;
    int64_t grad_numel = 0;

    // build(bump, fill) lays the parameters out: a count pass (fill = false), then over the arena, registering the slots
    template <class Build>
    mdt_status alloc(Build build, const char* what) {
        Bump count;
        build(count, false);
        hipError_t e = hipMalloc((void**)&arena, count.off * sizeof(float));
        if (e != hipSuccess) return mdt_fail(MDT_ERR_HIP, "hipMalloc(%s arena) failed: %s", what, hipGetErrorString(e));
        Bump real;
        real.base = arena;
        build(real, true);
        size_t mx = 0;
        for (const Slot& s : slots) mx = std::max(mx, (size_t)s.numel);
        e = hipMalloc((void**)&staging, mx * sizeof(float));
        if (e != hipSuccess) return mdt_fail(MDT_ERR_HIP, "hipMalloc(staging) failed: %s", hipGetErrorString(e));
        return MDT_OK;
    }
    void free_params() {
        (void)hipFree(wt_arena);
        (void)hipFree(arena);
        (void)hipFree(staging);
    }
    mdt_status load(const char* fn, const char* name, const float* src, int64_t numel, hipStream_t s) {
        Slot* slot = mdt_find_slot(slots, name);
        if (!slot) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: unknown parameter '%s'", fn, name);
        MDT_TRY(mdt_check_numel(fn, name, numel, *slot));
        const float* dev = nullptr;
        MDT_TRY(mdt_upload_slot(*slot, src, numel, staging, s, &dev));
        if (dev == staging) HIP_TRY(hipStreamSynchronize(s));  // the staging buffer is reused by the next upload
        slot->loaded = true;
        return MDT_OK;
    }
    // training: a W^T image for every Linear a slot packs into; every slot then needs a new upload
    mdt_status prepare_wt() {
        std::vector<Lin*> lins;
        for (Slot& sl : slots)
            if (sl.lin && std::find(lins.begin(), lins.end(), sl.lin) == lins.end()) lins.push_back(sl.lin);
        Bump count;
        for (Lin* l : lins) count.take((size_t)l->N * l->K);
        HIP_TRY(hipMalloc((void**)&wt_arena, count.off * sizeof(float)));
        Bump real;
        real.base = wt_arena;
        for (Lin* l : lins) l->wt = real.take((size_t)l->N * l->K);
        for (Slot& sl : slots) sl.loaded = false;
        return MDT_OK;
    }
    int64_t size() const { return (int64_t)slots.size(); }
    const char* name(int64_t i) const { return (i >= 0 && i < size()) ? slots[i].name.c_str() : nullptr; }
    int64_t numel(int64_t i) const { return (i >= 0 && i < size()) ? slots[i].numel : -1; }
    int64_t grad_total() const { return wt_arena ? grad_numel : -1; }
    int64_t grad_offset(int64_t i) const { return (wt_arena && i >= 0 && i < (int64_t)grad_off.size()) ? grad_off[i] : -1; }
    // the gradient of the parameter whose image starts at dst
    float* grad_of(float* grads, const float* dst) const {
        for (size_t i = 0; i < slots.size(); ++i)
            if (slots[i].dst == dst) return grads + grad_off[i];
        return nullptr;
    }
};

// ------------------------------------------------------------------------------------------------
// batch-sized device blocks
// ------------------------------------------------------------------------------------------------
// One block sized on demand for (need0, need1): on growth each dimension becomes the larger of the held and the needed size,
// the device is synchronised (earlier work may still read the old block), the block freed and reallocated through
// mdt_dev_malloc.  carve(bump, cap0, cap1) lays the buffers out over the block at the held capacity, on every call.
template <class Carve>
static mdt_status mdt_grow_carve(float*& buf, int64_t& cap0, int64_t& cap1, int64_t need0, int64_t need1, Carve carve) {
    if (need0 > cap0 || need1 > cap1) {
        const int64_t n0 = std::max(need0, cap0), n1 = std::max(need1, cap1);
        if (buf) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(mdt_dev_free(buf));
            buf = nullptr;
            cap0 = cap1 = 0;
        }
        Bump count;
        carve(count, n0, n1);
        HIP_TRY(mdt_dev_malloc((void**)&buf, count.off * sizeof(float)));
        cap0 = n0;
        cap1 = n1;
    }
    Bump real;
    real.base = buf;
    carve(real, cap0, cap1);
    return MDT_OK;
}

template <class Carve>  // the same for a block sized by the batch alone: carve(bump, cap)
static mdt_status mdt_grow_carve(float*& buf, int64_t& cap, int64_t need, Carve carve) {
    int64_t one = 1;
    return mdt_grow_carve(buf, cap, one, need, 1, [&](Bump& b, int64_t c, int64_t) { carve(b, c); });
}

// ------------------------------------------------------------------------------------------------
// training tapes
// ------------------------------------------------------------------------------------------------
struct TapeBase {
    bool in_use = false;
    // stream of the last call that read or wrote the tape, and the event release() records on it: a later forward that reuses
    // the buffers from ANOTHER stream waits for it (the release only marks the tape free on the host)
    hipStream_t stream = nullptr;
    hipEvent_t freed = nullptr;
    bool freed_pending = false;

    mdt_status release() {
        // the backward that last read the tape may still be in flight on its stream: leave a marker there for the next user
        if (!freed) HIP_TRY(hipEventCreateWithFlags(&freed, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(freed, stream));
        freed_pending = true;
        in_use = false;
        return MDT_OK;
    }
    void destroy_event() {
        if (freed) (void)hipEventDestroy(freed);
        freed = nullptr;
    }
};

// A tape of the pool for a forward on stream s: a free one that fits(tape) already, else any free one, else a new one while
// fewer than `limit` exist.  prepare(tape) sizes and carves its buffers; the tape is then in use on s.
template <class T, class Fits, class Prepare>
static mdt_status mdt_tape_acquire(std::vector<T>& pool, size_t limit, const char* what, hipStream_t s, Fits fits,
                                   Prepare prepare, int32_t* id) {
    int pick = -1;
    for (size_t i = 0; i < pool.size() && pick < 0; ++i)
        if (!pool[i].in_use && fits(pool[i])) pick = (int)i;
    for (size_t i = 0; i < pool.size() && pick < 0; ++i)
        if (!pool[i].in_use) pick = (int)i;
    if (pick < 0) {
        if (pool.size() >= limit)
            return mdt_fail(MDT_ERR_STATE, "more than %d %s alive: release tapes after their backward", (int)limit, what);
        pool.emplace_back();
        pick = (int)pool.size() - 1;
    }
    T& t = pool[pick];
    MDT_TRY(prepare(t));
    if (t.freed_pending && t.stream != s) HIP_TRY(hipStreamWaitEvent(s, t.freed, 0));  // its last reader ran elsewhere
    t.freed_pending = false;
    t.stream = s;
    t.in_use = true;
    *id = pick;
    return MDT_OK;
}

// "invalid or released <what> <id>" unless id names a tape in use
template <class T>
static mdt_status mdt_tape_get(std::vector<T>& pool, int32_t id, const char* what, T** out) {
    if (id < 0 || id >= (int)pool.size() || !pool[id].in_use)
        return mdt_fail(MDT_ERR_INVALID_ARG, "invalid or released %s %d", what, id);
    *out = &pool[id];
    return MDT_OK;
}
