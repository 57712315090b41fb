// C-ABI of libmythril_hip (include/mythril_hip.h): handles, error reporting, device buffers,
// launch orchestration.  No exception crosses the ABI and nothing here aborts the process:
// every failure is an MH_E_* code plus a thread-local message, so the Python front end can fall
// back to z3 (SURVEY.md §5 "fail closed").
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/mythril_hip.h"
#include "compile.h"
#include "dev_isa.h"
#include "domains.h"
#include "jit.h"
#include "kernels.h"
#include "launch_plan.h"
#include "values_plan.h"

constexpr uint32_t kSideStreams = 3;  // with the ctx stream: GPU_MAX_HW_QUEUES (4) queues

// MH_FANOUT=0 turns the short-run fan-out over side streams off (read once per process)
static bool fanout_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("MH_FANOUT");
        return !(e && e[0] == '0');
    }();
    return on;
}

struct AsyncCompile;  // mh_tapes_compile_async's worker (below)

struct mh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t* scratch = nullptr;  // microbench sink
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;  // one per timed sieve launch
    // per-query latency path (mh_run / mh_eval_values / mh_assign_download): grow-only device
    // result buffer and pinned host staging, so a query allocates nothing
    void* d_buf = nullptr;
    size_t d_buf_bytes = 0;
    void* h_buf = nullptr;
    size_t h_buf_bytes = 0;
    // multi-GPU: one RCCL communicator per handle (mh_comm_init)
    ncclComm_t comm = nullptr;
    int32_t rank = 0, world = 1;
    // device blocks of destroyed tape sets, by power-of-two size class: a query's tape set
    // reuses them instead of calling hipMalloc (a new size class costs milliseconds)
    std::unordered_map<size_t, std::vector<void*>> pool;
    std::unordered_map<void*, size_t> pool_class;
    size_t pool_bytes = 0;
    // tape sets and assignment buffers hold the context: mh_ctx_destroy before them only marks
    // it released, and the last child's destroy frees it
    int32_t children = 0;
    bool released = false;
    // pinned staging of tape-set uploads (one async copy per compile; the next compile waits on
    // the event before it refills the buffer)
    void* h_stage = nullptr;
    size_t h_stage_bytes = 0;
    hipEvent_t stage_ev = nullptr;
    bool stage_pending = false;
    // compiled tapes by content (the tape's nodes, the values of the constants it reads, the
    // column count): a LASER query's groups mostly repeat its parent's (svm.py:257-262), and a
    // tape's instruction words are self-contained (constants inline), so a repeated tape reuses
    // its words; cleared beyond kCacheWords words (mh_tapes_compile) or by mh_ctx_clear_cache
    std::unordered_map<std::string, std::pair<std::vector<uint32_t>, mh::CompiledTape>> compile_cache;
    size_t compile_cache_words = 0;
    // a short run's launches (one per register class) are a few waves each walking a long tape:
    // latency-bound, so they overlap on side streams (forked from and joined back into `stream`
    // by events) instead of queueing behind each other; created on first use
    hipStream_t side[kSideStreams] = {};
    hipEvent_t fork_ev = nullptr, join_ev[kSideStreams] = {};
    // the wave masks of a conjunct-parallel short run (grow-only)
    unsigned long long* d_masks = nullptr;
    size_t masks_bytes = 0;
    // mh_tapes_compile_async: one worker thread, started on first use, joined by ctx_free
    AsyncCompile* acomp = nullptr;
    // kernel launches of mh_eval_values_many (Model.eval batching is measured by it)
    uint64_t eval_launches = 0;
    // mh_query_round_many: the jobs' descriptors, block tables and packed guides go up in one
    // copy from this pinned staging area to this device block (both grow-only; the call ends with
    // a stream sync, so the next call finds the staging area free)
    void* h_batch = nullptr;
    void* d_batch = nullptr;
    size_t h_batch_bytes = 0, d_batch_bytes = 0;
    // the spill areas of the launches that run spilling tapes (F_SPILL, kernels.h KParams::spill):
    // grow-only, sized per call before anything of the call is queued (spill_reserve); the
    // launches of one call that may overlap take disjoint regions of it, and a later call's
    // launches are ordered after them (the side streams fork from and join into `stream`)
    uint32_t* d_spill = nullptr;
    size_t spill_bytes = 0;
    // the wave masks of a hit-listing run (mh_run_hits; grow-only).  Not d_masks: a split-tape run
    // writes that one.
    unsigned long long* d_hit_masks = nullptr;
    size_t hit_masks_bytes = 0;
};

// One compile at a time, handed to a worker thread that waits on a condition variable (a thread
// per call would cost its creation; a Python thread costs GIL hand-offs around the native call)
struct AsyncCompile {
    std::mutex m;
    std::condition_variable cv;
    std::thread th;
    bool stop = false, job = false, done = false;
    const mh_node* nodes = nullptr;
    const uint64_t* offs = nullptr;
    uint32_t n_tapes = 0, n_consts = 0, n_vars = 0;
    const uint32_t* consts = nullptr;
    int32_t rc = MH_OK;
    std::string err;
    mh_tapeset* out = nullptr;
    double seconds = 0;
};

namespace {
// RCCL is opened on first use (dlopen), not linked: a process that never shards never loads it.
// The ROCm install's copy comes first, opened by path with its own symbol scope (DEEPBIND): it
// binds to the same libamdhip64.so.7 this library runs on, whereas a Python wheel's bundled
// librccl (torch's) binds to the wheel's own HIP runtime -- on the box that copy fails with
// "no ROCm-capable device" when this library initialised HIP first.
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                               hipStream_t) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
};
const Rccl* rccl() {
    static Rccl r;
    static bool tried = false;
    if (!tried) {
        tried = true;
        // MH_RCCL_LIB names another copy first (a recording stub in tests/test_comm_stub.py)
        const char* env = std::getenv("MH_RCCL_LIB");
        for (const char* name : {env, "/opt/rocm/lib/librccl.so.1", "librccl.so.1"}) {
            if (!name || !*name) continue;
            r.h = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
            if (r.h || name == env) break;  // a named copy that fails is not replaced
        }
        if (r.h) {
            r.get_unique_id = (decltype(r.get_unique_id))dlsym(r.h, "ncclGetUniqueId");
            r.comm_init_rank = (decltype(r.comm_init_rank))dlsym(r.h, "ncclCommInitRank");
            r.all_reduce = (decltype(r.all_reduce))dlsym(r.h, "ncclAllReduce");
            r.comm_destroy = (decltype(r.comm_destroy))dlsym(r.h, "ncclCommDestroy");
            r.error_string = (decltype(r.error_string))dlsym(r.h, "ncclGetErrorString");
        }
    }
    if (!r.get_unique_id || !r.comm_init_rank || !r.all_reduce || !r.comm_destroy) return nullptr;
    return &r;
}
}  // namespace

namespace {
// A grow-only buffer (*p of *have bytes, device or pinned host memory) made to hold `bytes`: kept
// when it does, else freed and allocated anew at `least` bytes doubled until they suffice.  The
// caller has made sure that nothing queued still uses the old block.
template <class T>
hipError_t grow_buf(T** p, size_t* have, size_t bytes, size_t least, bool pinned) {
    if (bytes <= *have) return hipSuccess;
    hipError_t e = !*p ? hipSuccess : pinned ? hipHostFree(*p) : hipFree(*p);
    if (e != hipSuccess) return e;
    *p = nullptr;
    *have = 0;
    size_t n = least;
    while (n < bytes) n <<= 1;
    void* q = nullptr;
    e = pinned ? hipHostMalloc(&q, n, hipHostMallocDefault) : hipMalloc(&q, n);
    if (e != hipSuccess) return e;
    *p = static_cast<T*>(q);
    *have = n;
    return hipSuccess;
}
hipError_t ctx_dbuf(mh_ctx* c, size_t bytes, void** out) {
    const hipError_t e = grow_buf(&c->d_buf, &c->d_buf_bytes, bytes, 1 << 16, false);
    *out = c->d_buf;
    return e;
}
// smallest class 256 KiB: a query's whole tape set fits one block, so after the first query every
// compile reuses a block (a hipMalloc of a size the process has not seen costs milliseconds)
size_t pool_size_class(size_t bytes) {
    size_t n = 256u << 10;
    while (n < bytes) n <<= 1;
    return n;
}
template <class T>
hipError_t pool_alloc(mh_ctx* c, T** out, size_t bytes) {
    const size_t k = pool_size_class(bytes);
    auto& fl = c->pool[k];
    if (!fl.empty()) {
        *out = static_cast<T*>(fl.back());
        fl.pop_back();
        c->pool_bytes -= k;
        return hipSuccess;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, k);
    if (e != hipSuccess) return e;
    c->pool_class[p] = k;
    *out = static_cast<T*>(p);
    return hipSuccess;
}
void pool_free(mh_ctx* c, void* p) {
    if (!p) return;
    auto it = c->pool_class.find(p);
    if (it == c->pool_class.end()) {
        (void)hipFree(p);
        return;
    }
    if (c->pool_bytes + it->second > (256u << 20)) {  // keep at most 256 MiB cached
        (void)hipFree(p);
        c->pool_class.erase(it);
        return;
    }
    c->pool[it->second].push_back(p);
    c->pool_bytes += it->second;
}
hipError_t ctx_hbuf(mh_ctx* c, size_t bytes, void** out) {
    const hipError_t e = grow_buf(&c->h_buf, &c->h_buf_bytes, bytes, 1 << 16, true);
    *out = c->h_buf;
    return e;
}
}  // namespace

struct mh_tapeset {
    mh_ctx* ctx = nullptr;
    uint32_t n_tapes = 0;
    uint32_t n_vars = 0;
    void* d_block = nullptr;  // one pool block: insns | ids | tapes | consts
    uint2* d_insns = nullptr;
    mh_dev_tape* d_tapes = nullptr;
    uint32_t* d_consts = nullptr;
    std::vector<mh_tape_info> info;
    // the tapes bucketed by kernel variant (launch_plan.h Buckets), and the id list on the device
    mh::Buckets all;
    uint32_t* d_all = nullptr;
    // host copy of the IR, for mh_tapes_jit
    std::vector<mh_node> h_nodes;
    std::vector<uint64_t> h_offs;
    std::vector<uint32_t> h_consts;
    // native-code path (mh_tapes_jit): one module per slice of tape groups; the interpreter's
    // buckets restricted to the tapes the JIT does not take
    struct JitMod {
        hipModule_t mod = nullptr, vmod = nullptr;
        hipFunction_t fn = nullptr, vfn = nullptr;
        uint32_t n_groups = 0;
        // the code object images stay alive as long as the modules: the HIP runtime may read
        // an image after hipModuleLoadData returns (lazy loading)
        std::vector<char> image, vimage;
    };
    std::vector<JitMod> jit;
    std::vector<uint8_t> jitted;
    bool has_jit = false;
    mh::Buckets rest;
    uint32_t* d_rest = nullptr;
    mh_jit_info jinfo{};
    uint64_t code_id = 0;   // mh::jit::code_id of the count kernels' module texts
    // conjunct-parallel short runs (mh_run_async): a long tape's root conjunction cut into parts
    // of consecutive conjuncts, each compiled as a tape of its own (ids n_tapes, n_tapes + 1, ..,
    // in the order of their tapes) and bucketed like the tapes; the buckets without the split
    // tapes; per split tape, ascending: (tape, first part id, parts)
    uint32_t n_parts = 0;
    mh::Buckets unsplit, parts;
    std::vector<uint32_t> split_tab;
    uint32_t *d_unsplit = nullptr, *d_parts = nullptr, *d_split = nullptr;
    // table lookups (MH_OP_LOOKUP): a tape that runs one (F_TABLE) makes the set runnable by
    // mh_eval_values_tables only; the (table id, key words) pairs the tapes' nodes name
    bool has_tables = false;
    std::vector<std::pair<uint32_t, uint32_t>> lookups;
    // spill slots per tape, the parts after the tapes (0: the tape does not spill; F_SPILL tapes
    // run in mh::kSpillVariant with a region of the ctx's spill memory)
    std::vector<uint32_t> spills;
};

// The device block the sets of one mh_tables_create_many share: freed with the last handle.
struct TablesBlock {
    uint32_t* d = nullptr;
    uint32_t refs = 0;
};

struct mh_tables {
    mh_ctx* ctx = nullptr;
    uint32_t* d = nullptr;          // the packed set (dev_isa.h layout)
    std::vector<uint32_t> nws;      // key words per table
    TablesBlock* block = nullptr;   // null: `d` is a pool block of this set alone
};

struct mh_assign {
    mh_ctx* ctx = nullptr;
    uint32_t n_vars = 0;
    uint64_t capacity = 0;
    uint64_t stride = 0;           // words between column-limbs (capacity + assign_pad_rows)
    uint32_t* d = nullptr;
    uint32_t* d_guide = nullptr;   // packed mh_guide (grow-only)
    size_t guide_words = 0;
    std::vector<uint32_t> h_guide; // host packing of the guide
    uint32_t* h_pinned = nullptr;  // pinned staging of the packed guide (grow-only)
    size_t pinned_words = 0;
    hipEvent_t staged = nullptr;   // recorded after the staging copy; reuse waits on it
    bool staged_pending = false;
    // mh_assign_scatter: cols | values, pinned staging and device copy (grow-only), with an event
    // of their own so that a scatter queued behind a generator does not wait for the guide's copy
    uint32_t* h_scatter = nullptr;
    uint32_t* d_scatter = nullptr;
    size_t h_scatter_bytes = 0, d_scatter_bytes = 0;
    hipEvent_t scattered = nullptr;
    bool scatter_pending = false;
};

namespace {

thread_local std::string g_err;

int32_t set_err(int32_t code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace

// mh_last_error text for the host-only entry points of other translation units (harvest.cpp)
int32_t mh_detail_set_err(int32_t code, const char* msg) { return set_err(code, msg); }

namespace {

#define MH_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return set_err(MH_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

bool is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

// The compile worker thread (mh_tapes_compile_async) sets this: its own calls into the ctx do not
// wait for themselves.
thread_local bool t_compile_worker = false;

// Every entry point that uses a ctx's state (device buffers, the compiled-tape cache, the staging
// buffer, the pool, the stream) passes here: while the ctx's worker thread runs a compile, the
// call waits for that compile to finish (its result stays for mh_tapes_compile_wait), so no two
// threads touch the ctx at once.  The host-only harvest the caller overlaps with the
// compile never enters a ctx.
void settle(const mh_ctx* ctx) {
    AsyncCompile* a = ctx->acomp;
    if (!a || t_compile_worker) return;
    std::unique_lock<std::mutex> lk(a->m);
    a->cv.wait(lk, [&] { return !a->job || a->done; });
}

int32_t use_device(const mh_ctx* ctx) {
    settle(ctx);
    MH_HIP(hipSetDevice(ctx->device));
    return MH_OK;
}

uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int32_t check_run_args(const mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first,
                       uint32_t tape_count, const mh_assign* as, uint64_t row_first,
                       uint64_t row_count, uint32_t mode) {
    if (!ctx || !ts || !as) return set_err(MH_E_INVALID, "null handle");
    if (ts->ctx != ctx || as->ctx != ctx) return set_err(MH_E_INVALID, "handles of another ctx");
    if ((uint64_t)tape_first + tape_count > ts->n_tapes)
        return set_err(MH_E_INVALID, "tape range out of bounds");
    if (row_first > as->capacity || row_count > as->capacity - row_first)
        return set_err(MH_E_INVALID, "row range out of bounds");
    if (as->n_vars < ts->n_vars)
        return set_err(MH_E_INVALID, "assignment buffer has fewer columns than the tapes use");
    if (mode != MH_MODE_FIRST_HIT && mode != MH_MODE_COUNT_ALL)
        return set_err(MH_E_INVALID, "bad mode");
    return MH_OK;
}

// Every entry point but mh_eval_values_tables: it has no table set for a lookup to read.
int32_t refuse_tables(const mh_tapeset* ts) {
    if (ts && ts->has_tables)
        return set_err(MH_E_UNSUPPORTED,
                       "the tape set holds table lookups (MH_OP_LOOKUP): only "
                       "mh_eval_values_tables runs it");
    return MH_OK;
}

// mh_eval_values_tables / mh_eval_values_jobs: every lookup of the tape set names a table of the
// set, with the table's key words.
int32_t check_tables(const mh_ctx* ctx, const mh_tapeset* ts, const mh_tables* tables) {
    if (tables->ctx != ctx) return set_err(MH_E_INVALID, "table set of another ctx");
    for (const auto& lk : ts->lookups) {
        if (lk.first >= tables->nws.size())
            return set_err(MH_E_INVALID, "a lookup names table " + std::to_string(lk.first) +
                                             ", the set has " +
                                             std::to_string(tables->nws.size()));
        if (lk.second != tables->nws[lk.first])
            return set_err(MH_E_INVALID, "a lookup's key has " + std::to_string(lk.second) +
                                             " words, table " + std::to_string(lk.first) +
                                             " has " + std::to_string(tables->nws[lk.first]));
    }
    return MH_OK;
}

// The batched entry points' pinned staging area and device block (mh_ctx::h_batch / d_batch),
// grown to `bytes`: a submission goes up in one copy.
int32_t ctx_batch_bufs(mh_ctx* ctx, size_t bytes) {
    MH_HIP(grow_buf(&ctx->h_batch, &ctx->h_batch_bytes, bytes, 1 << 16, true));
    MH_HIP(grow_buf(&ctx->d_batch, &ctx->d_batch_bytes, bytes, 1 << 16, false));
    return MH_OK;
}

// Makes the ctx's spill memory hold `words` words: a call's mh::SpillPlan (launch_plan.h), the
// regions its spilling launches took while it was planned.  Called before a call queues anything: a
// call whose spill areas exceed the cap (256 MiB; MH_SPILL_CAP_MB for experiments) is refused whole.
// The memory grows only here, after everything queued on the ctx's streams has finished, so no
// launch can still be using the block that is freed.
int32_t spill_reserve(mh_ctx* ctx, uint64_t words) {
    if (words == 0) return MH_OK;
    static const uint64_t cap = [] {
        const char* e = std::getenv("MH_SPILL_CAP_MB");
        const uint64_t mb = e ? std::strtoull(e, nullptr, 10) : 0;
        return (mb ? mb : 256ull) << 20;
    }();
    const uint64_t bytes = words * sizeof(uint32_t);
    if (bytes > cap)
        return set_err(MH_E_UNSUPPORTED,
                       "the launch's spill areas take " + std::to_string(bytes) +
                           " bytes, more than the cap of " + std::to_string(cap) +
                           " (tapes with more live values than registers; fewer rows per run fit)");
    if (bytes <= ctx->spill_bytes) return MH_OK;
    MH_HIP(hipStreamSynchronize(ctx->stream));
    for (hipStream_t sd : ctx->side)
        if (sd) MH_HIP(hipStreamSynchronize(sd));
    const hipError_t e = grow_buf(&ctx->d_spill, &ctx->spill_bytes, bytes, (size_t)1 << 20, false);
    if (e != hipSuccess)
        return set_err(MH_E_NOMEM, std::string("spill memory: ") + hipGetErrorString(e));
    return MH_OK;
}

// a planned launch's spill fields (mh::plan_launches) in its KParams
void bind_spill(mh::KParams& q, const mh_ctx* ctx, const mh::Launch& l) {
    if (l.variant != mh::kSpillVariant) return;
    q.spill = ctx->d_spill + l.spill_off;
    q.spill_slots = l.spill_slots;
}

inline uint32_t seg_variant(const mh::batch::Segment& sg) { return sg.last_bucket; }
inline uint32_t seg_variant(const mh::values::Segment& sg) { return sg.variant; }
// The spill tail of a batched submission (mh_query_round_many, mh_eval_values_jobs), after the
// segments' KParams are made and before anything is queued.  At most one launch runs the spill
// variant (a register class of its own); its region is sized by its workgroups (one wave each, the
// area picked by the launch's workgroup index) times the most slots a tape of its segments uses,
// and every such segment names that region and slot count.  seg_tapes(sg) = the segment's tape
// set and its first id in the host's id list.
template <class Plan, class SegTapes>
int32_t batch_spill(mh_ctx* ctx, const Plan& plan, mh::KParams* h_seg, SegTapes seg_tapes) {
    uint32_t slots = 0;
    for (const auto& sg : plan.segments)
        if (seg_variant(sg) == mh::kSpillVariant) {
            const std::pair<const mh_tapeset*, const uint32_t*> t = seg_tapes(sg);
            for (uint32_t i = 0; i < sg.n_ids; ++i)
                slots = std::max(slots, t.first->spills[t.second[i]]);
        }
    mh::SpillPlan spill;
    for (const auto& l : plan.launches)
        if (l.variant == mh::kSpillVariant) (void)spill.take(l.count, slots);
    if (int32_t r = spill_reserve(ctx, spill.words)) return r;
    for (size_t si = 0; si < plan.segments.size(); ++si)
        if (seg_variant(plan.segments[si]) == mh::kSpillVariant) {
            h_seg[si].spill = ctx->d_spill;
            h_seg[si].spill_slots = slots;
        }
    return MH_OK;
}

// One timed span of launches on the ctx stream (mh_ctx_kernel_time sums them): nothing unless
// timing is on
hipError_t span_begin(mh_ctx* ctx) {
    if (!ctx->timing) return hipSuccess;
    std::pair<hipEvent_t, hipEvent_t> sp{nullptr, nullptr};
    hipError_t e = hipEventCreate(&sp.first);
    if (e == hipSuccess) e = hipEventCreate(&sp.second);
    if (e != hipSuccess) return e;
    ctx->spans.push_back(sp);
    return hipEventRecord(sp.first, ctx->stream);
}
hipError_t span_end(mh_ctx* ctx) {
    return ctx->timing ? hipEventRecord(ctx->spans.back().second, ctx->stream) : hipSuccess;
}

mh::KParams make_params(const mh_tapeset* ts, uint32_t tape_first, const mh_assign* as,
                        uint64_t row_first, uint64_t row_count, uint64_t index_base,
                        uint32_t mode) {
    mh::KParams p{};
    p.insns = ts->d_insns;
    p.tapes = ts->d_tapes;
    p.consts = ts->d_consts;
    p.assign = as->d;
    p.capacity = as->stride;
    p.n_pre = ts->n_vars <= MH_MAX_PRELOAD ? ts->n_vars : 0;
    p.result_base = tape_first;
    p.row_first = row_first;
    p.row_count = row_count;
    p.index_base = index_base;
    p.mode = mode;
    return p;
}

// Rows per workgroup of the JIT kernels: 4 waves, each over a contiguous run of 64-row chunks.
uint32_t jit_rows_per_wg(uint64_t row_count) {
    static const uint32_t forced = [] {  // diagnostic: MH_JIT_ROWS_PER_WG (multiple of 256)
        const char* e = std::getenv("MH_JIT_ROWS_PER_WG");
        const uint32_t v = e ? (uint32_t)atoi(e) : 0u;
        return (v >= 256 && v % 256 == 0) ? v : 0u;
    }();
    if (forced) return forced;
    uint64_t r = 256;
    while (r < 16384 && r * 2048 < row_count) r *= 2;  // >= ~2048 row blocks before growing
    return (uint32_t)r;
}

int32_t launch_jit(mh_ctx* ctx, const mh_tapeset* ts, const mh_assign* as, uint64_t row_first,
                   uint64_t row_count, uint64_t index_base, uint32_t mode, uint64_t* d_first_hit,
                   uint64_t* d_hit_count, uint32_t* d_values) {
    mh::jit::KernArgs a{};
    a.assign = (uint64_t)(uintptr_t)as->d;
    a.capacity = as->stride;
    a.row_first = row_first;
    a.row_count = row_count;
    a.index_base = index_base;
    a.first_hit = (uint64_t)(uintptr_t)d_first_hit;
    a.hit_count = (uint64_t)(uintptr_t)d_hit_count;
    a.rows_per_wg = jit_rows_per_wg(row_count);
    a.n_rowblocks = (uint32_t)((row_count + a.rows_per_wg - 1) / a.rows_per_wg);
    a.values_out = (uint64_t)(uintptr_t)d_values;
    a.mode = mode;
    if (as->stride >= (1ull << 30) || row_first + row_count > (1ull << 31))
        return set_err(MH_E_UNSUPPORTED, "JIT kernels address < 2^30 rows per column");
    for (const auto& j : ts->jit) {
        hipFunction_t fn = d_values ? j.vfn : j.fn;
        if (!fn || !j.n_groups) continue;
        for (uint32_t g0 = 0; g0 < j.n_groups; g0 += 65535) {
            a.group_first = g0;
            const uint32_t gy = std::min<uint32_t>(65535, j.n_groups - g0);
            size_t sz = sizeof(a);
            void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                           HIP_LAUNCH_PARAM_END};
            MH_HIP(hipModuleLaunchKernel(fn, a.n_rowblocks, gy, 1, 256, 1, 1, 0, ctx->stream,
                                         nullptr, cfg));
        }
    }
    return MH_OK;
}

}  // namespace

static int32_t eval_values_rows(mh_ctx* ctx, const mh_tapeset* ts, const mh_tables* tables,
                                const uint32_t* tapes, uint32_t n, const mh_assign* as,
                                uint64_t row, uint64_t row_count, uint32_t* out, const char* who,
                                bool single);

extern "C" {

int32_t mh_version(uint32_t* major, uint32_t* minor, uint32_t* patch) {
    if (major) *major = MH_VERSION_MAJOR;
    if (minor) *minor = MH_VERSION_MINOR;
    if (patch) *patch = MH_VERSION_PATCH;
    return MH_OK;
}

const char* mh_last_error(void) { return g_err.c_str(); }

int32_t mh_device_count(int32_t* n) {
    if (!n) return set_err(MH_E_INVALID, "null out pointer");
    *n = 0;
    int total = 0;
    if (hipGetDeviceCount(&total) != hipSuccess) {
        (void)hipGetLastError();
        return MH_OK;
    }
    for (int d = 0; d < total; ++d) *n += is_gfx950(d) ? 1 : 0;
    return MH_OK;
}

namespace {
void ctx_free(mh_ctx* ctx);
}

int32_t mh_ctx_create(int32_t device, mh_ctx** out) {
    if (!out) return set_err(MH_E_INVALID, "null out pointer");
    *out = nullptr;
    int total = 0;
    if (hipGetDeviceCount(&total) != hipSuccess || device < 0 || device >= total) {
        (void)hipGetLastError();
        return set_err(MH_E_NODEVICE, "no HIP device " + std::to_string(device));
    }
    if (!is_gfx950(device)) return set_err(MH_E_NODEVICE, "device is not gfx950 (MI355X)");
    mh_ctx* c = new (std::nothrow) mh_ctx();
    if (!c) return set_err(MH_E_NOMEM, "ctx allocation");
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    c->own_stream = c->stream != nullptr;
    // the short-run fan-out's side streams and events up front, when the fan-out is on: a stream
    // created on first use took 14.4 ms inside the query that first needed it (profiles/r04x).
    // With MH_FANOUT=0 a ctx holds its one stream (hardware queues are few per process)
    for (uint32_t i = 0; i < kSideStreams && e == hipSuccess && fanout_enabled(); ++i) {
        e = hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming);
    }
    if (e == hipSuccess && fanout_enabled())
        e = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&c->scratch, 64);
    if (e == hipSuccess) {
        // one block of the smallest class ready for the first query, and the pinned upload
        // staging; one round trip through them initialises the runtime's copy path for sizes a
        // query's first large tape set would otherwise pay for (~30 ms once per process)
        void* blk = nullptr;
        const size_t warm = 256u << 10;
        e = pool_alloc(c, (char**)&blk, warm);
        if (e == hipSuccess) e = hipHostMalloc(&c->h_stage, 1u << 20, hipHostMallocDefault);
        if (e == hipSuccess) {
            c->h_stage_bytes = 1u << 20;
            std::memset(c->h_stage, 0, warm);
            e = hipMemcpyAsync(blk, c->h_stage, warm, hipMemcpyHostToDevice, c->stream);
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->h_stage, blk, warm, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (blk) pool_free(c, blk);
    }
    if (e != hipSuccess) {
        ctx_free(c);
        return set_err(MH_E_DEVICE, std::string("ctx init: ") + hipGetErrorString(e));
    }
    *out = c;
    return MH_OK;
}

namespace {
void ctx_free(mh_ctx* ctx) {
    if (AsyncCompile* a = ctx->acomp) {
        {
            std::unique_lock<std::mutex> lk(a->m);
            a->cv.wait(lk, [&] { return !a->job || a->done; });  // a pending compile finishes
            a->stop = true;
        }
        a->cv.notify_all();
        if (a->th.joinable()) a->th.join();
        delete a;
        ctx->acomp = nullptr;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto& sp : ctx->spans) {
        (void)hipEventDestroy(sp.first);
        (void)hipEventDestroy(sp.second);
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (uint32_t i = 0; i < kSideStreams; ++i) {
        if (ctx->side[i]) {
            (void)hipStreamSynchronize(ctx->side[i]);
            (void)hipStreamDestroy(ctx->side[i]);
        }
        if (ctx->join_ev[i]) (void)hipEventDestroy(ctx->join_ev[i]);
    }
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    if (ctx->d_masks) (void)hipFree(ctx->d_masks);
    if (ctx->d_spill) (void)hipFree(ctx->d_spill);
    if (ctx->d_hit_masks) (void)hipFree(ctx->d_hit_masks);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->d_buf) (void)hipFree(ctx->d_buf);
    if (ctx->h_buf) (void)hipHostFree(ctx->h_buf);
    if (ctx->h_batch) (void)hipHostFree(ctx->h_batch);
    if (ctx->d_batch) (void)hipFree(ctx->d_batch);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->stage_ev) (void)hipEventDestroy(ctx->stage_ev);
    if (ctx->comm && rccl()) (void)rccl()->comm_destroy(ctx->comm);
    for (auto& kv : ctx->pool_class) (void)hipFree(kv.first);
    delete ctx;
}
// a child (tape set / assignment buffer) of `ctx` is gone
void ctx_unref(mh_ctx* ctx) {
    if (--ctx->children == 0 && ctx->released) ctx_free(ctx);
}
}  // namespace

int32_t mh_ctx_destroy(mh_ctx* ctx) {
    if (!ctx) return MH_OK;
    if (ctx->released) return set_err(MH_E_INVALID, "context already destroyed");
    if (AsyncCompile* a = ctx->acomp) {  // a compile nobody collected: finish and drop it
        mh_tapeset* left = nullptr;
        {
            std::unique_lock<std::mutex> lk(a->m);
            a->cv.wait(lk, [&] { return !a->job || a->done; });
            if (a->job) {
                left = a->out;
                a->out = nullptr;
                a->job = false;
            }
        }
        if (left) (void)mh_tapes_destroy(left);
    }
    if (ctx->children > 0) {
        ctx->released = true;
        return MH_OK;
    }
    ctx_free(ctx);
    return MH_OK;
}

int32_t mh_ctx_clear_cache(mh_ctx* ctx) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    settle(ctx);
    ctx->compile_cache.clear();
    ctx->compile_cache_words = 0;
    return MH_OK;
}

int32_t mh_ctx_set_stream(mh_ctx* ctx, void* hip_stream) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    if (int32_t r = use_device(ctx)) return r;
    // uploads queued on the current stream (tape sets, guides: asynchronous copies from pinned
    // staging) must land before anything on the new stream reads them
    MH_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) MH_HIP(hipStreamDestroy(ctx->stream));
    ctx->stream = (hipStream_t)hip_stream;  // NULL = the device's null stream
    ctx->own_stream = false;
    return MH_OK;
}

int32_t mh_ctx_synchronize(mh_ctx* ctx) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    if (int32_t r = use_device(ctx)) return r;
    MH_HIP(hipStreamSynchronize(ctx->stream));
    return MH_OK;
}

int32_t mh_tapes_compile_async(mh_ctx* ctx, const mh_node* nodes, const uint64_t* tape_offsets,
                               uint32_t n_tapes, const uint32_t* consts, uint32_t n_consts,
                               uint32_t n_vars) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    try {
        if (!ctx->acomp) {
            AsyncCompile* a = new AsyncCompile();
            a->th = std::thread([ctx, a] {
                t_compile_worker = true;
                std::unique_lock<std::mutex> lk(a->m);
                for (;;) {
                    a->cv.wait(lk, [&] { return a->stop || (a->job && !a->done); });
                    if (a->stop) return;
                    lk.unlock();
                    mh_tapeset* out = nullptr;
                    const auto t0 = std::chrono::steady_clock::now();
                    const int32_t rc = mh_tapes_compile(ctx, a->nodes, a->offs, a->n_tapes,
                                                        a->consts, a->n_consts, a->n_vars, &out);
                    const double dt = std::chrono::duration<double>(
                                          std::chrono::steady_clock::now() - t0).count();
                    const std::string err = rc == MH_OK ? std::string() : mh_last_error();
                    lk.lock();
                    a->rc = rc;
                    a->err = err;
                    a->out = out;
                    a->seconds = dt;
                    a->done = true;
                    a->cv.notify_all();
                }
            });
            ctx->acomp = a;
        }
    } catch (const std::exception&) {
        return set_err(MH_E_NOMEM, "compile worker thread");
    }
    AsyncCompile* a = ctx->acomp;
    {
        std::lock_guard<std::mutex> lk(a->m);
        if (a->job) return set_err(MH_E_INVALID, "a compile is already pending on this ctx");
        a->nodes = nodes;
        a->offs = tape_offsets;
        a->n_tapes = n_tapes;
        a->consts = consts;
        a->n_consts = n_consts;
        a->n_vars = n_vars;
        a->out = nullptr;
        a->rc = MH_OK;
        a->done = false;
        a->job = true;
    }
    a->cv.notify_all();
    return MH_OK;
}

int32_t mh_tapes_compile_wait(mh_ctx* ctx, mh_tapeset** out, double* compile_s) {
    if (!ctx || !out) return set_err(MH_E_INVALID, "null argument");
    *out = nullptr;
    AsyncCompile* a = ctx->acomp;
    if (!a) return set_err(MH_E_INVALID, "no compile pending on this ctx");
    std::unique_lock<std::mutex> lk(a->m);
    if (!a->job) return set_err(MH_E_INVALID, "no compile pending on this ctx");
    a->cv.wait(lk, [&] { return a->done; });
    a->job = false;
    *out = a->out;
    a->out = nullptr;
    if (compile_s) *compile_s = a->seconds;
    if (a->rc != MH_OK) return set_err(a->rc, a->err);
    return MH_OK;
}

int32_t mh_tapes_compile(mh_ctx* ctx, const mh_node* nodes, const uint64_t* tape_offsets,
                         uint32_t n_tapes, const uint32_t* consts, uint32_t n_consts,
                         uint32_t n_vars, mh_tapeset** out) {
    static const bool trace = std::getenv("MH_TRACE_COMPILE") != nullptr;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    const auto t_start = tnow();
    if (!ctx || !out || (!nodes && n_tapes) || !tape_offsets || (!consts && n_consts))
        return set_err(MH_E_INVALID, "null argument");
    *out = nullptr;
    settle(ctx);  // the compile cache, staging buffer and pool are the ctx's
    std::vector<uint32_t> words, dconsts;
    mh::ConstIndex dindex;
    std::vector<mh_dev_tape> heads(n_tapes);
    std::vector<mh_tape_info> info(n_tapes);
    std::vector<uint32_t> spills(n_tapes, 0);  // slots per tape, then per part
    // the buckets of the tapes, and of the conjunct-parallel parts (mh_tapeset): heads n_tapes..
    mh::Buckets bk_all, bk_unsplit, bk_parts;
    std::vector<uint32_t> split_tab;
    try {
        std::vector<std::vector<uint32_t>> tw(n_tapes);
        static const bool use_cache = [] {
            const char* e = std::getenv("MH_COMPILE_CACHE");
            return !(e && e[0] == '0');
        }();
        constexpr size_t kCacheWords = (size_t)16 << 20;  // 128 MB of instruction words
        std::string key;
        // one tape's words and summary, from the cache when its content was compiled before
        auto compile_one = [&](const mh_node* tn, size_t nn, std::vector<uint32_t>& w,
                               mh::CompiledTape& ct, std::string& err) -> int32_t {
            if (use_cache) {  // the tape's content: nodes, constant values, column count
                key.assign(reinterpret_cast<const char*>(&n_vars), sizeof n_vars);
                key.append(reinterpret_cast<const char*>(tn), nn * sizeof(mh_node));
                for (size_t i = 0; i < nn; ++i)
                    if (tn[i].op == MH_OP_CONST && tn[i].imm0 < n_consts)
                        key.append(reinterpret_cast<const char*>(consts + 8ull * tn[i].imm0), 32);
                auto hit = ctx->compile_cache.find(key);
                if (hit != ctx->compile_cache.end()) {
                    w = hit->second.first;
                    ct = hit->second.second;
                    return MH_OK;
                }
            }
            const int32_t r = mh::compile_tape(tn, nn, consts, n_consts, n_vars, dconsts, dindex,
                                               w, ct, err, true);
            if (r == MH_OK && use_cache) {
                if (ctx->compile_cache_words + w.size() > kCacheWords) {
                    ctx->compile_cache.clear();
                    ctx->compile_cache_words = 0;
                }
                ctx->compile_cache_words += w.size();
                ctx->compile_cache.emplace(key, std::make_pair(w, ct));
            }
            return r;
        };
        for (uint32_t t = 0; t < n_tapes; ++t) {
            const uint64_t b = tape_offsets[t], e = tape_offsets[t + 1];
            if (e <= b) return set_err(MH_E_INVALID, "tape " + std::to_string(t) + " is empty");
            mh::CompiledTape ct;
            std::string err;
            const int32_t r = compile_one(nodes + b, (size_t)(e - b), tw[t], ct, err);
            if (r != MH_OK) return set_err(r, "tape " + std::to_string(t) + ": " + err);
            heads[t] = mh_dev_tape{0, ct.n_insns, ct.root_bool, ct.n_regs};
            info[t] = mh_tape_info{ct.n_nodes, ct.n_insns, ct.n_regs, ct.features, ct.alg_ops};
            spills[t] = ct.n_spills;
        }
        // conjunct-parallel parts of the long tapes (a query round's latency is its longest
        // tape walked by one wave per SIMD: parts walk in parallel, mh_run_async); MH_SPLIT_INSNS
        // = the instruction slots from which a tape is cut, one part per that many.  Off by
        // default: measured on the LASER-shaped queries and paths, the parts' compile
        // costs a LASER child about what the parallel walk saves, and the 2^16-row miss round
        // pays the parts' duplicated sub-terms
        const char* se = std::getenv("MH_SPLIT_INSNS");
        const uint32_t split_min = se ? (uint32_t)std::strtoul(se, nullptr, 10) : 0u;
        constexpr uint32_t kMaxParts = 8;
        std::vector<std::vector<uint32_t>> pw;
        std::vector<mh_tape_info> pinfo;
        std::vector<mh_dev_tape> pheads;
        std::vector<uint32_t> pspills;
        for (uint32_t t = 0; split_min && t < n_tapes; ++t) {
            if (info[t].n_insns < split_min || !heads[t].root_bool) continue;
            if (info[t].features & F_TABLE) continue;  // never run by mh_run_async
            const uint64_t b = tape_offsets[t], e = tape_offsets[t + 1];
            const uint32_t want = std::min<uint32_t>(kMaxParts, (info[t].n_insns + split_min - 1) / split_min);
            std::vector<std::vector<mh_node>> parts;
            if (!mh::split_conjunction(nodes + b, (uint32_t)(e - b), std::max<uint32_t>(want, 2), parts))
                continue;
            const size_t p0 = pw.size();
            bool ok = true;
            for (const auto& tp : parts) {
                std::vector<uint32_t> w;
                mh::CompiledTape ct;
                std::string err;
                if (compile_one(tp.data(), tp.size(), w, ct, err) != MH_OK || !ct.root_bool) {
                    ok = false;  // (register pressure of a part, say): the tape runs whole
                    break;
                }
                pw.push_back(std::move(w));
                pinfo.push_back(mh_tape_info{ct.n_nodes, ct.n_insns, ct.n_regs, ct.features, ct.alg_ops});
                pheads.push_back(mh_dev_tape{0, ct.n_insns, ct.root_bool, ct.n_regs});
                pspills.push_back(ct.n_spills);
            }
            if (!ok) {
                pw.resize(p0);
                pinfo.resize(p0);
                pheads.resize(p0);
                pspills.resize(p0);
                continue;
            }
            split_tab.insert(split_tab.end(), {t, n_tapes + (uint32_t)p0, (uint32_t)parts.size()});
        }
        // bucket by kernel variant; instruction words laid out bucket by bucket (ascending tape
        // id inside a bucket) so that any run of consecutive bucket entries is one contiguous
        // range of words, which the kernel stages into LDS with one coalesced copy; the parts
        // after the tapes, likewise
        std::vector<char> is_split(n_tapes, 0);
        for (size_t i = 0; i < split_tab.size(); i += 3) is_split[split_tab[i]] = 1;
        heads.insert(heads.end(), pheads.begin(), pheads.end());
        spills.insert(spills.end(), pspills.begin(), pspills.end());
        const auto variant = [&](uint32_t t) {  // of a tape, or of the part with id t
            const mh_tape_info& ti = t < n_tapes ? info[t] : pinfo[t - n_tapes];
            return mh::variant_of(ti.n_regs, ti.features);
        };
        const auto every = [](uint32_t) { return true; };
        bk_all = mh::Buckets::build(n_tapes, 0, variant, every);
        bk_unsplit = mh::Buckets::build(n_tapes, 0, variant, [&](uint32_t t) { return !is_split[t]; });
        bk_parts = mh::Buckets::build((uint32_t)pw.size(), n_tapes,
                                      [&](uint32_t i) { return variant(n_tapes + i); }, every);
        for (const mh::Buckets* bk : {&bk_all, &bk_parts})
            for (uint32_t t : bk->ids) {
                const std::vector<uint32_t>& w = t < n_tapes ? tw[t] : pw[t - n_tapes];
                heads[t].insn_off = (uint32_t)(words.size() / 2);
                words.insert(words.end(), w.begin(), w.end());
            }
    } catch (const std::bad_alloc&) {
        return set_err(MH_E_NOMEM, "host allocation during compile");
    }
    const auto t_compiled = tnow();
    if (dconsts.empty()) dconsts.assign(8, 0);
    if (words.empty()) words.assign(2, 0);
    // the asm core's scalar prefetch reads the 8 slots from the next instruction on (its words and
    // its inline constants): zero slots after the last tape keep those loads inside the buffer
    words.resize(words.size() + 2 * 8, 0u);
    if (int32_t r = use_device(ctx)) return r;
    mh_tapeset* ts = new (std::nothrow) mh_tapeset();
    if (!ts) return set_err(MH_E_NOMEM, "tapeset allocation");
    ts->ctx = ctx;
    ++ctx->children;
    ts->n_tapes = n_tapes;
    ts->n_vars = n_vars;
    try {
        ts->h_nodes.assign(nodes, nodes + (n_tapes ? tape_offsets[n_tapes] : 0));
        ts->h_offs.assign(tape_offsets, tape_offsets + n_tapes + 1);
        ts->h_consts.assign(consts, consts + (size_t)n_consts * 8);
    } catch (const std::bad_alloc&) {
        mh_tapes_destroy(ts);
        return set_err(MH_E_NOMEM, "host copy of the tapes");
    }
    ts->all = std::move(bk_all);
    ts->unsplit = std::move(bk_unsplit);
    ts->parts = std::move(bk_parts);
    ts->info = std::move(info);
    ts->spills = std::move(spills);
    for (const mh_tape_info& ti : ts->info) ts->has_tables |= (ti.features & F_TABLE) != 0;
    for (uint32_t t = 0; t < n_tapes; ++t)
        mh::tape_lookups(nodes + tape_offsets[t], (size_t)(tape_offsets[t + 1] - tape_offsets[t]),
                         ts->lookups);
    ts->n_parts = (uint32_t)ts->parts.ids.size();
    ts->split_tab = std::move(split_tab);
    // one device block and one async copy from pinned staging (a query compiles a tape set per
    // call: four synchronous pageable copies cost more than the kernels they feed)
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    auto b_u32 = [](const std::vector<uint32_t>& v) { return std::max<size_t>(1, v.size()) * 4; };
    const size_t b_insns = words.size() * sizeof(uint32_t), b_ids = b_u32(ts->all.ids),
                 b_tapes = std::max<size_t>(1, heads.size()) * sizeof(mh_dev_tape),
                 b_consts = dconsts.size() * sizeof(uint32_t);
    const size_t o_ids = al(b_insns), o_tapes = o_ids + al(b_ids), o_consts = o_tapes + al(b_tapes),
                 o_unsplit = o_consts + al(b_consts), o_parts = o_unsplit + al(b_u32(ts->unsplit.ids)),
                 o_split = o_parts + al(b_u32(ts->parts.ids)),
                 total = o_split + al(b_u32(ts->split_tab));
    hipError_t e = pool_alloc(ctx, (char**)&ts->d_block, total);
    if (e == hipSuccess && ctx->stage_pending) {
        e = hipEventSynchronize(ctx->stage_ev);
        ctx->stage_pending = false;
    }
    if (e == hipSuccess && total > ctx->h_stage_bytes) {
        const size_t n = std::max<size_t>({total, 2 * ctx->h_stage_bytes, (size_t)1 << 20});
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
        ctx->h_stage = nullptr;
        ctx->h_stage_bytes = 0;
        e = hipHostMalloc(&ctx->h_stage, n, hipHostMallocDefault);
        if (e == hipSuccess) ctx->h_stage_bytes = n;
    }
    if (e == hipSuccess && !ctx->stage_ev)
        e = hipEventCreateWithFlags(&ctx->stage_ev, hipEventDisableTiming);
    if (e == hipSuccess) {
        char* h = (char*)ctx->h_stage;
        std::memcpy(h, words.data(), b_insns);
        if (!heads.empty()) std::memcpy(h + o_tapes, heads.data(), heads.size() * sizeof(mh_dev_tape));
        std::memcpy(h + o_consts, dconsts.data(), b_consts);
        auto put = [&](size_t o, const std::vector<uint32_t>& v) {
            if (!v.empty()) std::memcpy(h + o, v.data(), v.size() * sizeof(uint32_t));
        };
        put(o_ids, ts->all.ids);
        put(o_unsplit, ts->unsplit.ids);
        put(o_parts, ts->parts.ids);
        put(o_split, ts->split_tab);
        char* d = (char*)ts->d_block;
        ts->d_insns = (uint2*)d;
        ts->d_all = (uint32_t*)(d + o_ids);
        ts->d_tapes = (mh_dev_tape*)(d + o_tapes);
        ts->d_consts = (uint32_t*)(d + o_consts);
        ts->d_unsplit = (uint32_t*)(d + o_unsplit);
        ts->d_parts = (uint32_t*)(d + o_parts);
        ts->d_split = (uint32_t*)(d + o_split);
        e = hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->stage_ev, ctx->stream);
        if (e == hipSuccess) ctx->stage_pending = true;
    }
    if (e != hipSuccess) {
        mh_tapes_destroy(ts);
        return set_err(MH_E_DEVICE, std::string("tapeset upload: ") + hipGetErrorString(e));
    }
    if (trace) {
        auto us = [](auto a, auto b) {
            return std::chrono::duration<double, std::micro>(b - a).count();
        };
        fprintf(stderr, "mh_tapes_compile: %u tapes, %zu words, compile %.1f us, upload %.1f us\n",
                n_tapes, words.size(), us(t_start, t_compiled), us(t_compiled, tnow()));
    }
    *out = ts;
    return MH_OK;
}

int32_t mh_tapes_destroy(mh_tapeset* ts) {
    if (!ts) return MH_OK;
    settle(ts->ctx);
    (void)hipSetDevice(ts->ctx->device);
    // kernels of this set may still run on the ctx stream: finish them before the blocks go back
    if (ts->ctx->stream) (void)hipStreamSynchronize(ts->ctx->stream);
    pool_free(ts->ctx, ts->d_block);
    if (ts->d_rest) (void)hipFree(ts->d_rest);
    for (auto& j : ts->jit) {
        if (j.mod) (void)hipModuleUnload(j.mod);
        if (j.vmod) (void)hipModuleUnload(j.vmod);
    }
    mh_ctx* ctx = ts->ctx;
    delete ts;
    ctx_unref(ctx);
    return MH_OK;
}

int32_t mh_tapes_spills(const mh_tapeset* ts, uint32_t* out, uint32_t n_tapes) {
    if (!ts || !out) return set_err(MH_E_INVALID, "null argument");
    if (n_tapes > ts->n_tapes) return set_err(MH_E_INVALID, "n_tapes exceeds the tape set");
    std::copy(ts->spills.begin(), ts->spills.begin() + n_tapes, out);
    return MH_OK;
}

int32_t mh_tapes_split_info(const mh_tapeset* ts, uint32_t* n_split, uint32_t* n_parts,
                            uint32_t* tape_parts, uint32_t n_tapes) {
    if (!ts) return set_err(MH_E_INVALID, "null argument");
    if (n_tapes > ts->n_tapes) return set_err(MH_E_INVALID, "n_tapes exceeds the tape set");
    if (n_split) *n_split = (uint32_t)(ts->split_tab.size() / 3);
    if (n_parts) *n_parts = ts->n_parts;
    if (tape_parts) {
        std::fill(tape_parts, tape_parts + n_tapes, 0u);
        for (size_t i = 0; i < ts->split_tab.size(); i += 3)
            if (ts->split_tab[i] < n_tapes) tape_parts[ts->split_tab[i]] = ts->split_tab[i + 2];
    }
    return MH_OK;
}

int32_t mh_tapes_info(const mh_tapeset* ts, mh_tape_info* info, uint32_t n_tapes) {
    if (!ts || !info) return set_err(MH_E_INVALID, "null argument");
    if (n_tapes > ts->n_tapes) return set_err(MH_E_INVALID, "n_tapes exceeds the tape set");
    std::copy(ts->info.begin(), ts->info.begin() + n_tapes, info);
    return MH_OK;
}

// Rows of padding after each column-limb.  The limbs of one row lie `stride` words apart; with
// a power-of-two stride (2^26 rows = 256 MiB) the 32 limbs a chunk loads alias in the address
// bits that pick the HBM channel.  MH_ASSIGN_PAD_ROWS overrides (A/B).
uint64_t assign_pad_rows(uint64_t capacity) {
    static const long long forced = [] {
        const char* e = std::getenv("MH_ASSIGN_PAD_ROWS");
        return e ? atoll(e) : -1ll;
    }();
    if (forced >= 0) return (uint64_t)forced;
    (void)capacity;
    return 0;
}

int32_t mh_assign_create(mh_ctx* ctx, uint32_t n_vars, uint64_t capacity, mh_assign** out) {
    if (!ctx || !out) return set_err(MH_E_INVALID, "null argument");
    *out = nullptr;
    if (n_vars == 0 || capacity == 0) return set_err(MH_E_INVALID, "empty assignment buffer");
    if (int32_t r = use_device(ctx)) return r;
    mh_assign* as = new (std::nothrow) mh_assign();
    if (!as) return set_err(MH_E_NOMEM, "assign allocation");
    as->ctx = ctx;
    ++ctx->children;
    as->n_vars = n_vars;
    as->capacity = capacity;
    as->stride = capacity + assign_pad_rows(capacity);
    hipError_t e = hipMalloc(&as->d, (size_t)n_vars * 8 * as->stride * sizeof(uint32_t));
    if (e != hipSuccess) {
        mh_assign_destroy(as);
        return set_err(MH_E_NOMEM, std::string("assignment buffer: ") + hipGetErrorString(e));
    }
    *out = as;
    return MH_OK;
}

int32_t mh_assign_destroy(mh_assign* as) {
    if (!as) return MH_OK;
    settle(as->ctx);
    (void)hipSetDevice(as->ctx->device);
    if (as->staged_pending) (void)hipEventSynchronize(as->staged);
    if (as->staged) (void)hipEventDestroy(as->staged);
    if (as->h_pinned) (void)hipHostFree(as->h_pinned);
    if (as->scatter_pending) (void)hipEventSynchronize(as->scattered);
    if (as->scattered) (void)hipEventDestroy(as->scattered);
    if (as->h_scatter) (void)hipHostFree(as->h_scatter);
    if (as->d_scatter) (void)hipFree(as->d_scatter);
    if (as->d) (void)hipFree(as->d);
    if (as->d_guide) (void)hipFree(as->d_guide);
    mh_ctx* ctx = as->ctx;
    delete as;
    ctx_unref(ctx);
    return MH_OK;
}

int32_t mh_tables_create(mh_ctx* ctx, uint32_t n_tables, const uint32_t* counts,
                         const uint32_t* nws, const uint64_t* key_offsets, const uint32_t* keys,
                         uint64_t n_key_limbs, const uint64_t* value_offsets,
                         const uint32_t* values, uint64_t n_value_limbs,
                         const uint32_t* else_values, mh_tables** out) {
    if (!ctx || !out) return set_err(MH_E_INVALID, "null argument");
    *out = nullptr;
    std::vector<uint32_t> packed;
    std::string err;
    try {
        if (int32_t r = mh::pack_tables(n_tables, counts, nws, key_offsets, keys, n_key_limbs,
                                        value_offsets, values, n_value_limbs, else_values, packed,
                                        err))
            return set_err(r, "mh_tables_create: " + err);
    } catch (const std::bad_alloc&) {
        return set_err(MH_E_NOMEM, "host allocation of the table set");
    }
    if (int32_t r = use_device(ctx)) return r;
    mh_tables* tb = new (std::nothrow) mh_tables();
    if (!tb) return set_err(MH_E_NOMEM, "table set allocation");
    tb->ctx = ctx;
    ++ctx->children;
    tb->nws.assign(nws, nws + n_tables);
    // a pool block like a tape set's: a certified hit allocates nothing after the first
    hipError_t e = pool_alloc(ctx, &tb->d, packed.size() * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpyAsync(tb->d, packed.data(), packed.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `packed` is pageable and local
    if (e != hipSuccess) {
        mh_tables_destroy(tb);
        return set_err(MH_E_DEVICE, std::string("table set upload: ") + hipGetErrorString(e));
    }
    *out = tb;
    return MH_OK;
}

int32_t mh_tables_create_many(mh_ctx* ctx, uint32_t n_sets, const uint32_t* set_tables,
                              const uint32_t* counts, const uint32_t* nws,
                              const uint64_t* key_offsets, const uint32_t* keys,
                              uint64_t n_key_limbs, const uint64_t* value_offsets,
                              const uint32_t* values, uint64_t n_value_limbs,
                              const uint32_t* else_values, mh_tables** out) {
    // host-only up to use_device(): one invalid set creates nothing
    if (!ctx || (n_sets && (!out || !set_tables)))
        return set_err(MH_E_INVALID, "mh_tables_create_many: null argument");
    for (uint32_t s = 0; s < n_sets; ++s) out[s] = nullptr;
    if (n_sets == 0) return MH_OK;
    std::vector<uint32_t> all, packed;
    std::vector<size_t> off(n_sets);  // words; every set starts 16-byte aligned
    std::vector<mh_tables*> made;
    const auto undo = [&] {
        for (mh_tables* t : made) {
            --ctx->children;
            delete t;
        }
    };
    try {
        size_t t0 = 0;
        for (uint32_t s = 0; s < n_sets; ++s) {
            const uint32_t nt = set_tables[s];
            std::string err;
            // set s's tables are entries [t0, t0 + nt) of the per-table arrays
            if (int32_t r = mh::pack_tables(nt, counts ? counts + t0 : nullptr, nws ? nws + t0 : nullptr,
                                            key_offsets ? key_offsets + t0 : nullptr, keys,
                                            n_key_limbs, value_offsets ? value_offsets + t0 : nullptr,
                                            values, n_value_limbs,
                                            else_values ? else_values + 8 * t0 : nullptr, packed,
                                            err)) {
                undo();
                return set_err(r, "mh_tables_create_many: set " + std::to_string(s) + ": " + err);
            }
            off[s] = all.size();
            all.insert(all.end(), packed.begin(), packed.end());
            all.resize((all.size() + 3) & ~(size_t)3, 0u);
            mh_tables* tb = new mh_tables();
            tb->ctx = ctx;
            ++ctx->children;
            made.push_back(tb);
            if (nt) tb->nws.assign(nws + t0, nws + t0 + nt);
            t0 += nt;
        }
    } catch (const std::bad_alloc&) {
        undo();
        return set_err(MH_E_NOMEM, "host allocation of the table sets");
    }
    if (int32_t r = use_device(ctx)) {
        undo();
        return r;
    }
    TablesBlock* blk = new (std::nothrow) TablesBlock();
    if (!blk) {
        undo();
        return set_err(MH_E_NOMEM, "table block allocation");
    }
    hipError_t e = pool_alloc(ctx, &blk->d, all.size() * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpyAsync(blk->d, all.data(), all.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `all` is pageable and local
    if (e != hipSuccess) {
        if (blk->d) pool_free(ctx, blk->d);
        delete blk;
        undo();
        return set_err(MH_E_DEVICE, std::string("table sets upload: ") + hipGetErrorString(e));
    }
    blk->refs = n_sets;
    for (uint32_t s = 0; s < n_sets; ++s) {
        made[s]->block = blk;
        made[s]->d = blk->d + off[s];
        out[s] = made[s];
    }
    return MH_OK;
}

int32_t mh_tables_destroy(mh_tables* tb) {
    if (!tb) return MH_OK;
    settle(tb->ctx);
    (void)hipSetDevice(tb->ctx->device);
    if (tb->ctx->stream) (void)hipStreamSynchronize(tb->ctx->stream);
    if (!tb->block) {
        pool_free(tb->ctx, tb->d);
    } else if (--tb->block->refs == 0) {
        pool_free(tb->ctx, tb->block->d);
        delete tb->block;
    }
    mh_ctx* ctx = tb->ctx;
    delete tb;
    ctx_unref(ctx);
    return MH_OK;
}

int32_t mh_assign_upload(mh_assign* as, const uint32_t* host_soa, uint64_t first, uint64_t count) {
    if (!as || (!host_soa && count)) return set_err(MH_E_INVALID, "null argument");
    if (first > as->capacity || count > as->capacity - first)
        return set_err(MH_E_INVALID, "row range out of bounds");
    if (int32_t r = use_device(as->ctx)) return r;
    if (count == 0) return MH_OK;
    // one strided copy into every column-limb's [first, first + count) slice: a definitions
    // evaluation uploads one row, which one copy per column-limb made 0.15 ms (profiles/r04z)
    MH_HIP(hipMemcpy2DAsync(as->d + first, as->stride * sizeof(uint32_t), host_soa,
                            count * sizeof(uint32_t), count * sizeof(uint32_t),
                            (size_t)as->n_vars * 8, hipMemcpyHostToDevice, as->ctx->stream));
    MH_HIP(hipStreamSynchronize(as->ctx->stream));
    return MH_OK;
}

int32_t mh_assign_download(const mh_assign* as, uint32_t* host_soa, uint64_t first,
                           uint64_t count) {
    if (!as || (!host_soa && count)) return set_err(MH_E_INVALID, "null argument");
    if (first > as->capacity || count > as->capacity - first)
        return set_err(MH_E_INVALID, "row range out of bounds");
    if (int32_t r = use_device(as->ctx)) return r;
    if (count == 0) return MH_OK;
    // one strided copy of every column-limb's [first, first + count) slice (a query reads one
    // witness row: one call instead of one per column-limb)
    MH_HIP(hipMemcpy2DAsync(host_soa, count * sizeof(uint32_t), as->d + first,
                            as->stride * sizeof(uint32_t), count * sizeof(uint32_t),
                            (size_t)as->n_vars * 8, hipMemcpyDeviceToHost, as->ctx->stream));
    MH_HIP(hipStreamSynchronize(as->ctx->stream));
    return MH_OK;
}

int32_t mh_assign_generate(mh_assign* as, uint64_t seed, uint64_t global_base) {
    if (!as) return set_err(MH_E_INVALID, "null handle");
    if (int32_t r = use_device(as->ctx)) return r;
    MH_HIP(mh::launch_generate(as->d, as->stride, as->capacity, as->n_vars, seed, global_base,
                               as->ctx->stream));
    return MH_OK;
}

// The packed form of a guide: width | pool_off | pool | set_prob | set_off | alt_off | entry_col |
// entry_val, in words.
struct GuideLayout {
    uint32_t nc = 0, ns = 0, n_pool = 0, n_alts = 0, n_ent = 0, n_value_sets = 0;
    size_t o_width = 0, o_poff = 0, o_pool = 0, o_prob = 0, o_soff = 0, o_aoff = 0, o_ecol = 0,
           o_eval = 0, words = 0;
};
// Every offset and entry of the guide checked on the host (the kernels trust them) and its
// layout: no device call.
static int32_t check_guide(const mh_assign* as, const mh_guide* g, GuideLayout* L) {
    if (g->n_cols > as->n_vars) return set_err(MH_E_INVALID, "guide has more columns than the buffer");
    if (g->n_cols && (!g->col_width || !g->pool_off))
        return set_err(MH_E_INVALID, "guide: null column arrays");
    if (g->n_sets && (!g->set_prob || !g->set_off || !g->alt_off))
        return set_err(MH_E_INVALID, "guide: null set arrays");
    // validate every offset and entry on the host: the kernel trusts them
    const uint32_t nc = g->n_cols, ns = g->n_sets;
    if (nc && g->pool_off[0] != 0) return set_err(MH_E_INVALID, "guide: pool_off[0] != 0");
    for (uint32_t v = 0; v < nc; ++v) {
        if (g->col_width[v] < 1 || g->col_width[v] > 256)
            return set_err(MH_E_INVALID, "guide: column width outside 1..256");
        if (g->pool_off[v + 1] < g->pool_off[v])
            return set_err(MH_E_INVALID, "guide: pool_off not monotone");
    }
    const uint32_t n_pool = nc ? g->pool_off[nc] : 0;
    if (n_pool && !g->pool) return set_err(MH_E_INVALID, "guide: null pool");
    const uint32_t n_alts = ns ? g->set_off[ns] : 0;
    if (ns && g->set_off[0] != 0) return set_err(MH_E_INVALID, "guide: set_off[0] != 0");
    for (uint32_t j = 0; j < ns; ++j)
        if (g->set_off[j + 1] < g->set_off[j])
            return set_err(MH_E_INVALID, "guide: set_off not monotone");
    if (ns && g->alt_off[0] != 0) return set_err(MH_E_INVALID, "guide: alt_off[0] != 0");
    for (uint32_t a = 0; a < n_alts; ++a)
        if (g->alt_off[a + 1] < g->alt_off[a])
            return set_err(MH_E_INVALID, "guide: alt_off not monotone");
    const uint32_t n_ent = ns ? g->alt_off[n_alts] : 0;
    if (n_ent && (!g->entry_col || !g->entry_val))
        return set_err(MH_E_INVALID, "guide: null entry arrays");
    // the leading sets without a copy entry (the kernel resolves their writes in LDS)
    uint32_t n_value_sets = 0;
    for (bool copy = false; n_value_sets < ns && !copy; ) {
        for (uint32_t e = g->alt_off[g->set_off[n_value_sets]];
             e < g->alt_off[g->set_off[n_value_sets + 1]] && !copy; ++e)
            copy = (g->entry_col[e] & MH_GUIDE_COPY) != 0;
        if (!copy) ++n_value_sets;
    }
    for (uint32_t e = 0; e < n_ent; ++e) {
        const uint32_t c = g->entry_col[e];
        const uint32_t dst = c & ~MH_GUIDE_COPY;
        if (dst >= nc) return set_err(MH_E_INVALID, "guide: entry column out of range");
        if (c & MH_GUIDE_COPY) {
            const uint32_t* ev = g->entry_val + (size_t)e * 8;
            if (ev[0] >= nc || ev[3] < 1 || ev[3] > 256 || ev[1] >= 256 || ev[2] >= 256)
                return set_err(MH_E_INVALID, "guide: malformed copy entry");
        }
    }
    L->nc = nc;
    L->ns = ns;
    L->n_pool = n_pool;
    L->n_alts = n_alts;
    L->n_ent = n_ent;
    L->n_value_sets = n_value_sets;
    L->o_width = 0;
    L->o_poff = L->o_width + nc;
    L->o_pool = L->o_poff + nc + 1;
    L->o_prob = L->o_pool + (size_t)n_pool * 8;
    L->o_soff = L->o_prob + ns;
    L->o_aoff = L->o_soff + ns + 1;
    L->o_ecol = L->o_aoff + n_alts + 1;
    L->o_eval = L->o_ecol + n_ent;
    L->words = L->o_eval + (size_t)n_ent * 8;
    return MH_OK;
}

// A checked guide packed into h[0, L.words)
static void pack_guide(const mh_guide* g, const GuideLayout& L, uint32_t* h) {
    const uint32_t nc = L.nc, ns = L.ns, n_pool = L.n_pool, n_alts = L.n_alts, n_ent = L.n_ent;
    std::fill(h, h + L.words, 0u);
    for (uint32_t v = 0; v < nc; ++v) h[L.o_width + v] = g->col_width[v];
    if (nc) std::copy(g->pool_off, g->pool_off + nc + 1, h + L.o_poff);
    if (n_pool) std::copy(g->pool, g->pool + (size_t)n_pool * 8, h + L.o_pool);
    for (uint32_t j = 0; j < ns; ++j) h[L.o_prob + j] = g->set_prob[j];
    if (ns) {
        std::copy(g->set_off, g->set_off + ns + 1, h + L.o_soff);
        std::copy(g->alt_off, g->alt_off + n_alts + 1, h + L.o_aoff);
    }
    if (n_ent) {
        std::copy(g->entry_col, g->entry_col + n_ent, h + L.o_ecol);
        std::copy(g->entry_val, g->entry_val + (size_t)n_ent * 8, h + L.o_eval);
    }
}

// The device form of a guide packed at `d`
static mh::KGuide guide_at(const GuideLayout& L, const uint32_t* d) {
    mh::KGuide k;
    k.n_cols = L.nc;
    k.n_sets = L.ns;
    k.n_value_sets = L.n_value_sets;
    k.width = d + L.o_width;
    k.pool_off = d + L.o_poff;
    k.pool = d + L.o_pool;
    k.set_prob = d + L.o_prob;
    k.set_off = d + L.o_soff;
    k.alt_off = d + L.o_aoff;
    k.entry_col = d + L.o_ecol;
    k.entry_val = d + L.o_eval;
    k.span_words = (uint32_t)(L.o_eval - L.o_prob);
    return k;
}

// The guide checked, packed and queued for upload into `as`'s guide buffer (on the ctx stream):
// *k = its device form.  Shared by the generator and the repair step's mutate (mh_repair_mutate).
static int32_t stage_guide(mh_assign* as, const mh_guide* g, mh::KGuide* out) {
    GuideLayout L;
    if (int32_t r = check_guide(as, g, &L)) return r;
    if (int32_t r = use_device(as->ctx)) return r;
    const size_t words = L.words;
    std::vector<uint32_t>& h = as->h_guide;
    h.resize(words);
    pack_guide(g, L, h.data());
    // both buffers grow geometrically: a LASER child's guide is a little larger than its
    // parent's, and a pinned reallocation per query cost ~0.24 ms (hipHostFree 0.19 +
    // hipHostMalloc 0.05, EtherThief-400, profiles/r05o/htrace)
    const size_t grow = std::max<size_t>({words, 2 * as->guide_words, (size_t)1 << 14});
    if (words > as->guide_words) {
        if (as->d_guide) MH_HIP(hipFree(as->d_guide));
        as->d_guide = nullptr;
        as->guide_words = 0;
        MH_HIP(hipMalloc(&as->d_guide, grow * sizeof(uint32_t)));
        as->guide_words = grow;
    }
    // pinned staging: the async copy needs no stream sync; the next call's packing waits on
    // the event of this copy before it overwrites the staging buffer
    if (as->staged_pending) {
        MH_HIP(hipEventSynchronize(as->staged));
        as->staged_pending = false;
    }
    if (words > as->pinned_words) {
        const size_t pgrow = std::max<size_t>({words, 2 * as->pinned_words, (size_t)1 << 14});
        if (as->h_pinned) MH_HIP(hipHostFree(as->h_pinned));
        as->h_pinned = nullptr;
        as->pinned_words = 0;
        MH_HIP(hipHostMalloc(&as->h_pinned, pgrow * sizeof(uint32_t), hipHostMallocDefault));
        as->pinned_words = pgrow;
    }
    if (!as->staged) MH_HIP(hipEventCreateWithFlags(&as->staged, hipEventDisableTiming));
    std::memcpy(as->h_pinned, h.data(), words * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(as->d_guide, as->h_pinned, words * sizeof(uint32_t),
                          hipMemcpyHostToDevice, as->ctx->stream));
    MH_HIP(hipEventRecord(as->staged, as->ctx->stream));
    as->staged_pending = true;
    *out = guide_at(L, as->d_guide);
    return MH_OK;
}

int32_t mh_assign_generate_guided(mh_assign* as, uint64_t seed, uint64_t global_base,
                                  uint64_t first, uint64_t count, const mh_guide* g) {
    if (!as || !g) return set_err(MH_E_INVALID, "null argument");
    if (first > as->capacity || count > as->capacity - first)
        return set_err(MH_E_INVALID, "row range out of bounds");
    mh::KGuide k;
    if (int32_t r = stage_guide(as, g, &k)) return r;
    MH_HIP(mh::launch_generate_guided(as->d, as->stride, first, count, seed, global_base, k,
                                      as->ctx->stream));
    return MH_OK;
}

uint32_t mh_gen_limb(uint64_t seed, uint32_t var, uint64_t index, uint32_t limb) {
    const uint64_t key = splitmix64(seed ^ (((uint64_t)var * 8 + limb) * 0xD1B54A32D192ED03ull));
    return (uint32_t)splitmix64(key ^ index);
}

int32_t mh_results_reset(mh_ctx* ctx, uint64_t* d_first_hit, uint64_t* d_hit_count, uint32_t n) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    if (int32_t r = use_device(ctx)) return r;
    // one small kernel for both arrays (two hipMemsetAsync were two fill launches per run)
    MH_HIP(mh::launch_results_reset(d_first_hit, d_hit_count, n, ctx->stream));
    return MH_OK;
}

// A complex-op interpreter tape over a buffer of 2^30 rows per column or more (kernels.h).
static int32_t refuse_capacity(uint64_t capacity) {
    return set_err(MH_E_UNSUPPORTED,
                   "interpreter tapes with complex ops (keccak, EVM helpers, overflow predicates, "
                   "loaded columns) address < 2^30 rows per column; this buffer's stride is " +
                   std::to_string(capacity) + " rows");
}

int32_t mh_run_async(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first, uint32_t tape_count,
                     const mh_assign* as, uint64_t row_first, uint64_t row_count,
                     uint64_t index_base, uint32_t mode, uint64_t* d_first_hit,
                     uint64_t* d_hit_count) {
    if (int32_t r = check_run_args(ctx, ts, tape_first, tape_count, as, row_first, row_count, mode))
        return r;
    if (int32_t r = refuse_tables(ts)) return r;
    if (int32_t r = use_device(ctx)) return r;
    mh::KParams p = make_params(ts, tape_first, as, row_first, row_count, index_base, mode);
    p.first_hit = reinterpret_cast<unsigned long long*>(d_first_hit);
    p.hit_count = reinterpret_cast<unsigned long long*>(d_hit_count);
    // the native code takes the jitted tapes of a whole-set run; the interpreter the rest
    const bool use_jit = ts->has_jit && tape_first == 0 && tape_count == ts->n_tapes;
    // a short interpreter run over a set with split tapes runs their parts instead (conjunct-
    // parallel: each part is a tape of its own, its waves write Bool masks, the combine kernel
    // ANDs them per split tape); MH_SPLIT_ROWS = the largest such run
    static const uint64_t split_rows = [] {
        const char* e = std::getenv("MH_SPLIT_ROWS");
        return e ? std::strtoull(e, nullptr, 10) : 65536ull;
    }();
    const bool split = !use_jit && ts->n_parts && row_count <= split_rows;
    const mh::Buckets& ids = use_jit ? ts->rest : split ? ts->unsplit : ts->all;
    const uint32_t* d_ids = use_jit ? ts->d_rest : split ? ts->d_unsplit : ts->d_all;
    // the split tapes inside the range (split_tab ascends by tape, part ids with it): their parts
    // are the ids [part_lo, part_hi)
    uint32_t s_lo = 0, s_hi = 0, part_lo = 0, part_hi = 0;
    if (split) {
        const uint32_t n_split = (uint32_t)ts->split_tab.size() / 3;
        while (s_lo < n_split && ts->split_tab[3 * s_lo] < tape_first) ++s_lo;
        s_hi = s_lo;
        while (s_hi < n_split && ts->split_tab[3 * s_hi] < tape_first + tape_count) ++s_hi;
        if (s_hi > s_lo) {
            part_lo = ts->split_tab[3 * s_lo + 1];
            part_hi = ts->split_tab[3 * (s_hi - 1) + 1] + ts->split_tab[3 * (s_hi - 1) + 2];
        }
    }
    // one launch per kernel-variant bucket; a short run (a query's guided first round) over the
    // whole set is one launch per register class instead (launch_plan.h plan_launches)
    static const uint64_t merge_rows = [] {
        const char* e = std::getenv("MH_MERGE_ROWS");
        return e ? std::strtoull(e, nullptr, 10) : 4096ull;
    }();
    const bool merge = !use_jit && row_count <= merge_rows && tape_first == 0 &&
                       tape_count == ts->n_tapes;
    // the launches of the whole tapes [0] and of the parts [1] (none unless `split`), a region of
    // spill memory for each that spills (they may overlap on the side streams): refused, and the
    // memory sized, before anything is queued
    mh::SpillPlan spill;
    const mh::LaunchPlan plans[2] = {
        mh::plan_launches(ids, tape_first, tape_count, row_count, merge, false, p.capacity,
                          ts->spills.data(), spill, mh::sieve_launch_waves),
        mh::plan_launches(ts->parts, part_lo, part_hi - part_lo, row_count, merge, true,
                          p.capacity, ts->spills.data(), spill, mh::sieve_launch_waves)};
    if (plans[0].misfit >= 0 || plans[1].misfit >= 0) return refuse_capacity(p.capacity);
    if (int32_t r = spill_reserve(ctx, spill.words)) return r;
    const uint64_t mask_stride = mh::sieve_mask_stride(row_count);
    MH_HIP(grow_buf(&ctx->d_masks, &ctx->masks_bytes,
                    (size_t)(part_hi - part_lo) * mask_stride * sizeof(unsigned long long),
                    1 << 16, false));
    MH_HIP(span_begin(ctx));
    if (use_jit && row_count) {
        if (int32_t r = launch_jit(ctx, ts, as, row_first, row_count, index_base, mode,
                                   d_first_hit, d_hit_count, nullptr))
            return r;
    }
    const uint32_t n_launch = plans[0].n + plans[1].n;
    // a short run's launches overlap on the side streams (made with the ctx when the fan-out
    // is on); the results they write are disjoint (per tape / per part), and the join puts
    // everything after them back in `stream`'s order
    const uint32_t n_side = fanout_enabled() && (merge || split)
                                ? std::min(n_launch - (n_launch > 0), kSideStreams) : 0;
    if (n_side) {
        MH_HIP(hipEventRecord(ctx->fork_ev, ctx->stream));
        for (uint32_t i = 0; i < n_side; ++i) MH_HIP(hipStreamWaitEvent(ctx->side[i], ctx->fork_ev, 0));
    }
    for (uint32_t i = 0; i < n_launch; ++i) {
        const bool part = i >= plans[0].n;
        const mh::Launch& l = part ? plans[1].launches[i - plans[0].n] : plans[0].launches[i];
        mh::KParams q = p;
        if (part) {  // wave masks instead of results
            q.masks = ctx->d_masks;
            q.mask_base = part_lo;
            q.mask_stride = mask_stride;
            q.first_hit = nullptr;
            q.hit_count = nullptr;
        }
        q.tape_ids = (part ? ts->d_parts : d_ids) + l.first;
        q.n_ids = l.count;
        bind_spill(q, ctx, l);
        // launch 0 on the ctx stream, the others round-robin over the side streams
        hipStream_t s = n_side && i ? ctx->side[(i - 1) % n_side] : ctx->stream;
        MH_HIP(mh::launch_sieve(q, l.variant, s));
    }
    for (uint32_t i = 0; i < n_side; ++i) {
        MH_HIP(hipEventRecord(ctx->join_ev[i], ctx->side[i]));
        MH_HIP(hipStreamWaitEvent(ctx->stream, ctx->join_ev[i], 0));
    }
    if (s_hi > s_lo)  // every part's masks written: the split tapes' results
        MH_HIP(mh::launch_combine(ctx->d_masks, mask_stride, ts->d_split + 3 * s_lo, s_hi - s_lo,
                                  part_lo, tape_first, index_base + row_first, p.first_hit,
                                  p.hit_count, ctx->stream));
    MH_HIP(span_end(ctx));
    return MH_OK;
}

int32_t mh_run_rows(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first, uint32_t tape_count,
                    const mh_assign* as, uint64_t row_first, uint64_t row_count,
                    uint64_t index_base, uint32_t mode, uint64_t* first_hit, uint64_t* hit_count,
                    uint32_t n_cols, uint32_t* rows_out) {
    if (int32_t r = check_run_args(ctx, ts, tape_first, tape_count, as, row_first, row_count, mode))
        return r;
    if (n_cols && (!rows_out || n_cols > as->n_vars))
        return set_err(MH_E_INVALID, "mh_run_rows: rows_out null or n_cols beyond the buffer's columns");
    if (int32_t r = refuse_tables(ts)) return r;
    if (int32_t r = use_device(ctx)) return r;
    const size_t n = std::max<uint32_t>(tape_count, 1);
    const size_t res_bytes = 2 * n * sizeof(uint64_t);
    const size_t row_bytes = (size_t)tape_count * n_cols * 8 * sizeof(uint32_t);
    void* dv = nullptr;
    void* hv = nullptr;
    MH_HIP(ctx_dbuf(ctx, res_bytes + row_bytes, &dv));
    MH_HIP(ctx_hbuf(ctx, res_bytes + row_bytes, &hv));
    uint64_t* d = static_cast<uint64_t*>(dv);
    uint64_t* h = static_cast<uint64_t*>(hv);
    int32_t r = mh_results_reset(ctx, d, d + n, (uint32_t)n);
    if (r == MH_OK)
        r = mh_run_async(ctx, ts, tape_first, tape_count, as, row_first, row_count, index_base,
                         mode, d, d + n);
    hipError_t e = hipSuccess;
    if (r == MH_OK && row_bytes)
        e = mh::launch_witness_rows(as->d, as->stride, d, tape_count, index_base, n_cols,
                                    reinterpret_cast<uint32_t*>(d + 2 * n), ctx->stream);
    if (r == MH_OK && e == hipSuccess)  // results and rows in one copy into pinned memory
        e = hipMemcpyAsync(h, d, res_bytes + row_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (r == MH_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (r == MH_OK && e == hipSuccess && first_hit && tape_count)
        std::memcpy(first_hit, h, tape_count * sizeof(uint64_t));
    if (r == MH_OK && e == hipSuccess && hit_count && tape_count)
        std::memcpy(hit_count, h + n, tape_count * sizeof(uint64_t));
    if (r == MH_OK && e == hipSuccess && row_bytes) std::memcpy(rows_out, h + 2 * n, row_bytes);
    if (r != MH_OK) return r;
    if (e != hipSuccess) return set_err(MH_E_DEVICE, std::string("mh_run: ") + hipGetErrorString(e));
    return MH_OK;
}

int32_t mh_run(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first, uint32_t tape_count,
               const mh_assign* as, uint64_t row_first, uint64_t row_count, uint64_t index_base,
               uint32_t mode, uint64_t* first_hit, uint64_t* hit_count) {
    return mh_run_rows(ctx, ts, tape_first, tape_count, as, row_first, row_count, index_base, mode,
                       first_hit, hit_count, 0, nullptr);
}

int32_t mh_query_round(mh_ctx* ctx, const mh_tapeset* ts, mh_assign* as, const mh_guide* guide,
                       uint64_t seed, uint64_t global_base, uint64_t count, uint32_t tape_first,
                       uint32_t tape_count, uint32_t mode, uint64_t* first_hit,
                       uint64_t* hit_count, uint32_t n_cols, uint32_t* rows_out) {
    if (!ctx || !as || as->ctx != ctx) return set_err(MH_E_INVALID, "null or foreign assignment buffer");
    if (int32_t r = check_run_args(ctx, ts, tape_first, tape_count, as, 0, count, mode)) return r;
    if (int32_t r = refuse_tables(ts)) return r;
    // the generator, the run and the copy queue back to back on the ctx stream: one host sync
    if (int32_t r = mh_assign_generate_guided(as, seed, global_base, 0, count, guide)) return r;
    return mh_run_rows(ctx, ts, tape_first, tape_count, as, 0, count, global_base, mode, first_hit,
                       hit_count, n_cols, rows_out);
}

// The device copy of a domain set: n KDomain descriptors, then the list values.  Made on the
// set's first use with a context and kept in the handle (domains.h) until mh_domains_free, or
// until the set is used with another context's buffer.
static void domains_release(mh_domains* d) {
    mh_ctx* ctx = static_cast<mh_ctx*>(d->dev_owner);
    if (d->dev) {
        settle(ctx);
        (void)hipSetDevice(ctx->device);
        (void)hipFree(d->dev);
    }
    d->dev = nullptr;
    d->dev_owner = nullptr;
    d->dev_release = nullptr;
    ctx_unref(ctx);
}

static int32_t domains_upload(mh_domains* d, mh_ctx* ctx) {
    if (d->dev && d->dev_owner == ctx) return MH_OK;
    if (d->dev_release) d->dev_release(d);
    const size_t n = d->cols.size();
    std::vector<mh::KDomain> h(n);
    for (size_t j = 0; j < n; ++j) {
        mh::KDomain& k = h[j];
        std::memset(&k, 0, sizeof k);
        k.size = d->size[j];
        k.col = d->cols[j];
        k.kind = d->kind[j];
        std::memcpy(k.lo, &d->lo[8 * j], sizeof k.lo);
        k.list_off = d->list_off[j];
    }
    const size_t desc_bytes = n * sizeof(mh::KDomain);
    const size_t val_bytes = d->list_vals.size() * sizeof(uint32_t);
    void* dev = nullptr;
    MH_HIP(hipMalloc(&dev, desc_bytes + std::max<size_t>(val_bytes, sizeof(uint32_t))));
    hipError_t e = hipMemcpy(dev, h.data(), desc_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && val_bytes)
        e = hipMemcpy(static_cast<char*>(dev) + desc_bytes, d->list_vals.data(), val_bytes,
                      hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return set_err(MH_E_DEVICE, std::string("domain upload: ") + hipGetErrorString(e));
    }
    d->dev = dev;
    d->dev_owner = ctx;
    d->dev_release = domains_release;
    ++ctx->children;
    return MH_OK;
}

int32_t mh_assign_enumerate(mh_assign* as, mh_domains* d, uint64_t global_base, uint64_t first,
                            uint64_t count) {
    // everything up to use_device() is host-only: a refused call has launched nothing
    if (!as || !d) return set_err(MH_E_INVALID, "mh_assign_enumerate: null argument");
    if (first > as->capacity || count > as->capacity - first)
        return set_err(MH_E_INVALID, "mh_assign_enumerate: row range out of bounds");
    if (global_base > d->rows || count > d->rows - global_base)
        return set_err(MH_E_INVALID, "mh_assign_enumerate: global_base + count exceeds the rows");
    for (uint32_t c : d->cols)
        if (c >= as->n_vars)
            return set_err(MH_E_INVALID, "mh_assign_enumerate: domain column " + std::to_string(c) +
                                             " beyond the buffer's columns");
    if (count == 0 || d->cols.empty()) return MH_OK;  // (a ground group: the one empty row)
    if (int32_t r = use_device(as->ctx)) return r;
    if (int32_t r = domains_upload(d, as->ctx)) return r;
    const size_t n = d->cols.size();
    const mh::KDomain* doms = static_cast<const mh::KDomain*>(d->dev);
    const uint32_t* vals = reinterpret_cast<const uint32_t*>(doms + n);
    MH_HIP(mh::launch_enumerate(as->d, as->stride, first, count, global_base, doms, (uint32_t)n,
                                vals, as->ctx->stream));
    return MH_OK;
}

int32_t mh_query_enumerate(mh_ctx* ctx, const mh_tapeset* ts, mh_assign* as, mh_domains* d,
                           uint64_t global_base, uint64_t count, uint32_t tape, uint32_t mode,
                           uint64_t* first_hit, uint64_t* hit_count, uint32_t n_cols,
                           uint32_t* rows_out) {
    if (!ctx || !as || as->ctx != ctx) return set_err(MH_E_INVALID, "null or foreign assignment buffer");
    if (!d) return set_err(MH_E_INVALID, "mh_query_enumerate: null domains");
    if (int32_t r = check_run_args(ctx, ts, tape, 1, as, 0, count, mode)) return r;
    if (n_cols && (!rows_out || n_cols > as->n_vars))
        return set_err(MH_E_INVALID, "mh_query_enumerate: rows_out null or n_cols beyond the buffer's columns");
    if (int32_t r = refuse_tables(ts)) return r;
    // the generator, the run and the copy queue back to back on the ctx stream: one host sync
    if (int32_t r = mh_assign_enumerate(as, d, global_base, 0, count)) return r;
    return mh_run_rows(ctx, ts, tape, 1, as, 0, count, global_base, mode, first_hit, hit_count,
                       n_cols, rows_out);
}

int32_t mh_query_round_many(mh_ctx* ctx, const mh_round_job* jobs, uint32_t n_jobs) {
    // everything below up to use_device() is host-only: a refused batch has queued nothing
    if (!ctx) return set_err(MH_E_INVALID, "mh_query_round_many: null ctx");
    if (n_jobs == 0) return MH_OK;
    if (n_jobs > MH_ROUND_MANY_MAX)
        return set_err(MH_E_INVALID, "mh_query_round_many: " + std::to_string(n_jobs) +
                                         " jobs, more than MH_ROUND_MANY_MAX (" +
                                         std::to_string(MH_ROUND_MANY_MAX) + "): chunk the list");
    if (!jobs) return set_err(MH_E_INVALID, "mh_query_round_many: null job list");
    const auto job_err = [](uint32_t i, int32_t code, const std::string& what) {
        return set_err(code, "mh_query_round_many: job " + std::to_string(i) + ": " + what);
    };
    struct JobPlan {
        GuideLayout L;
        mh::Buckets::Range in[mh::kNumVariants];  // the job's tapes per bucket
        size_t guide_off = 0, res_off = 0;  // words of the device block / bytes of the results
    };
    std::vector<JobPlan> jp(n_jobs);
    std::vector<mh::batch::JobShape> shapes(n_jobs);
    size_t res_bytes = 0;
    uint32_t max_tc = 0;
    bool any_rows = false;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_job& j = jobs[i];
        if (!j.ts || !j.as || !j.guide) return job_err(i, MH_E_INVALID, "null handle");
        if (j.ts->ctx != ctx || j.as->ctx != ctx)
            return job_err(i, MH_E_INVALID, "handles of another ctx");
        for (uint32_t k = 0; k < i; ++k)
            if (jobs[k].as == j.as)
                return job_err(i, MH_E_INVALID, "shares its assignment buffer with job " +
                                                    std::to_string(k));
        if (j.count > mh::batch::kMaxRows)
            return job_err(i, MH_E_UNSUPPORTED, std::to_string(j.count) + " rows, more than " +
                                                    std::to_string(mh::batch::kMaxRows));
        if (j.count > j.as->capacity)
            return job_err(i, MH_E_UNSUPPORTED, std::to_string(j.count) +
                                                    " rows, more than the buffer's capacity");
        if (int32_t r = check_run_args(ctx, j.ts, j.tape_first, j.tape_count, j.as, 0, j.count,
                                       j.mode))
            return job_err(i, r, g_err);
        if (j.n_cols && (!j.rows_out || j.n_cols > j.as->n_vars))
            return job_err(i, MH_E_INVALID, "rows_out null or n_cols beyond the buffer's columns");
        if (int32_t r = refuse_tables(j.ts)) return job_err(i, r, g_err);
        if (int32_t r = check_guide(j.as, j.guide, &jp[i].L)) return job_err(i, r, g_err);
        // the job's tapes per interpreter bucket: whole tapes (ts->all), never split parts
        mh::batch::JobShape& sh = shapes[i];
        sh.count = j.count;
        sh.whole = j.tape_first == 0 && j.tape_count == j.ts->n_tapes;
        sh.gen_n_cols = jp[i].L.nc;
        sh.gen_span_words = (uint32_t)(jp[i].L.o_eval - jp[i].L.o_prob);
        for (uint32_t v = 0; v < mh::kNumVariants; ++v) {
            jp[i].in[v] = j.ts->all.range(v, j.tape_first, j.tape_count);
            sh.n_ids[v] = jp[i].in[v].count;
        }
        jp[i].res_off = res_bytes;
        res_bytes += 2 * (size_t)j.tape_count * sizeof(uint64_t) +
                     (size_t)j.tape_count * j.n_cols * 8 * sizeof(uint32_t);
        max_tc = std::max(max_tc, j.tape_count);
        any_rows = any_rows || (j.n_cols && j.tape_count);
    }
    // (a job without tapes has no segment, but the generator still writes its rows, as
    // mh_query_round's does)
    const mh::batch::Plan plan = mh::batch::plan(shapes.data(), n_jobs);
    const mh::batch::Plan& gplan = plan;
    // a launch's variant serves every segment in it: each must fit that segment's buffer
    for (const auto& l : plan.launches)
        for (uint32_t b = l.first; b < l.first + l.count; ++b) {
            const uint32_t job = plan.segments[plan.blocks[b].seg].job;
            if (!mh::variant_fits(l.variant, jobs[job].as->stride)) {
                (void)refuse_capacity(jobs[job].as->stride);
                return job_err(job, MH_E_UNSUPPORTED, g_err);
            }
        }
    // the device block: segments' KParams | GenJob[] | ResultJob[] | block tables | guides
    const auto align = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_seg = 0;
    const size_t o_gen = align(o_seg + plan.segments.size() * sizeof(mh::KParams));
    const size_t o_res = align(o_gen + n_jobs * sizeof(mh::GenJob));
    const size_t o_blk = align(o_res + n_jobs * sizeof(mh::ResultJob));
    const size_t o_gblk = align(o_blk + plan.blocks.size() * sizeof(mh::batch::BlockEntry));
    size_t up_bytes = align(o_gblk + gplan.gen_blocks.size() * sizeof(mh::batch::GenEntry));
    for (uint32_t i = 0; i < n_jobs; ++i) {
        jp[i].guide_off = up_bytes;
        up_bytes = align(up_bytes + jp[i].L.words * sizeof(uint32_t));
    }
    if (int32_t r = use_device(ctx)) return r;
    if (int32_t r = ctx_batch_bufs(ctx, up_bytes)) return r;
    void* dres_v = nullptr;
    void* hres_v = nullptr;
    MH_HIP(ctx_dbuf(ctx, std::max<size_t>(res_bytes, 8), &dres_v));
    MH_HIP(ctx_hbuf(ctx, std::max<size_t>(res_bytes, 8), &hres_v));
    char* const dres = static_cast<char*>(dres_v);
    const char* const hres = static_cast<const char*>(hres_v);
    char* const hb = static_cast<char*>(ctx->h_batch);
    char* const db = static_cast<char*>(ctx->d_batch);
    // fill the staging area
    mh::GenJob* h_gen = reinterpret_cast<mh::GenJob*>(hb + o_gen);
    mh::ResultJob* h_res = reinterpret_cast<mh::ResultJob*>(hb + o_res);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_job& j = jobs[i];
        pack_guide(j.guide, jp[i].L, reinterpret_cast<uint32_t*>(hb + jp[i].guide_off));
        mh::GenJob g{};
        g.assign = j.as->d;
        g.stride = j.as->stride;
        g.count = j.count;
        g.seed = j.seed;
        g.base = j.global_base;
        g.g = guide_at(jp[i].L, reinterpret_cast<const uint32_t*>(db + jp[i].guide_off));
        h_gen[i] = g;
        mh::ResultJob r{};
        r.first_hit = reinterpret_cast<uint64_t*>(dres + jp[i].res_off);
        r.assign = j.as->d;
        r.stride = j.as->stride;
        r.index_base = j.global_base;
        r.tc = j.tape_count;
        r.n_cols = j.n_cols;
        h_res[i] = r;
    }
    mh::KParams* h_seg = reinterpret_cast<mh::KParams*>(hb + o_seg);
    for (size_t si = 0; si < plan.segments.size(); ++si) {
        const mh::batch::Segment& sg = plan.segments[si];
        const mh_round_job& j = jobs[sg.job];
        mh::KParams p = make_params(j.ts, j.tape_first, j.as, 0, j.count, j.global_base, j.mode);
        unsigned long long* fh = reinterpret_cast<unsigned long long*>(dres + jp[sg.job].res_off);
        p.first_hit = fh;
        p.hit_count = fh + j.tape_count;
        p.tape_ids = j.ts->d_all + jp[sg.job].in[sg.first_bucket].first;
        p.n_ids = sg.n_ids;
        h_seg[si] = p;
    }
    if (int32_t r = batch_spill(ctx, plan, h_seg, [&](const mh::batch::Segment& sg) {
            const mh_tapeset* ts = jobs[sg.job].ts;
            return std::make_pair(ts, ts->all.ids.data() + jp[sg.job].in[sg.first_bucket].first);
        }))
        return r;
    if (!plan.blocks.empty())
        std::memcpy(hb + o_blk, plan.blocks.data(),
                    plan.blocks.size() * sizeof(mh::batch::BlockEntry));
    if (!gplan.gen_blocks.empty())
        std::memcpy(hb + o_gblk, gplan.gen_blocks.data(),
                    gplan.gen_blocks.size() * sizeof(mh::batch::GenEntry));
    MH_HIP(span_begin(ctx));  // one span for the whole submission
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(db, hb, up_bytes, hipMemcpyHostToDevice, s);
    const mh::GenJob* d_gen = reinterpret_cast<const mh::GenJob*>(db + o_gen);
    const mh::ResultJob* d_res = reinterpret_cast<const mh::ResultJob*>(db + o_res);
    const mh::batch::GenEntry* d_gblk = reinterpret_cast<const mh::batch::GenEntry*>(db + o_gblk);
    const mh::batch::BlockEntry* d_blk = reinterpret_cast<const mh::batch::BlockEntry*>(db + o_blk);
    for (const auto& l : gplan.gen_launches)
        if (e == hipSuccess)
            e = mh::launch_generate_guided_batch(d_gen, d_gblk + l.first, l.count, l.form,
                                                 l.lds_bytes, s);
    if (e == hipSuccess && max_tc) e = mh::launch_results_reset_batch(d_res, n_jobs, s);
    for (const auto& l : plan.launches)
        if (e == hipSuccess)
            e = mh::launch_sieve_batch(reinterpret_cast<const mh::KParams*>(db + o_seg),
                                       d_blk + l.first, l.count, l.variant, s);
    if (e == hipSuccess && any_rows) e = mh::launch_witness_rows_batch(d_res, n_jobs, max_tc, s);
    if (e == hipSuccess) e = span_end(ctx);
    if (e == hipSuccess && res_bytes)
        e = hipMemcpyAsync(hres_v, dres, res_bytes, hipMemcpyDeviceToHost, s);
    // the staging area is read by the queued copy: wait even after an error
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess)
        return set_err(MH_E_DEVICE, std::string("mh_query_round_many: ") + hipGetErrorString(e));
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_job& j = jobs[i];
        const size_t tc = j.tape_count;
        const char* h = hres + jp[i].res_off;
        if (j.first_hit && tc) std::memcpy(j.first_hit, h, tc * sizeof(uint64_t));
        if (j.hit_count && tc)
            std::memcpy(j.hit_count, h + tc * sizeof(uint64_t), tc * sizeof(uint64_t));
        if (j.n_cols && tc)
            std::memcpy(j.rows_out, h + 2 * tc * sizeof(uint64_t),
                        tc * j.n_cols * 8 * sizeof(uint32_t));
    }
    return MH_OK;
}

int32_t mh_eval_values(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape, const mh_assign* as,
                       uint64_t row_first, uint64_t row_count, uint32_t* out) {
    if (int32_t r = check_run_args(ctx, ts, tape, 1, as, row_first, row_count, MH_MODE_COUNT_ALL))
        return r;
    if (!out && row_count) return set_err(MH_E_INVALID, "null out");
    if (int32_t r = refuse_tables(ts)) return r;
    // the one-tape list, without the list entry points' 2^31-word refusal and launch count
    return eval_values_rows(ctx, ts, nullptr, &tape, 1, as, row_first, row_count, out,
                            "mh_eval_values", true);
}

int32_t mh_eval_values_many(mh_ctx* ctx, const mh_tapeset* ts, const uint32_t* tapes,
                            uint32_t n, const mh_assign* as, uint64_t row, uint32_t* out) {
    return eval_values_rows(ctx, ts, nullptr, tapes, n, as, row, 1, out, "mh_eval_values_many",
                            false);
}

int32_t mh_eval_values_tables(mh_ctx* ctx, const mh_tapeset* ts, const mh_tables* tables,
                              const uint32_t* tapes, uint32_t n, const mh_assign* as,
                              uint64_t row_first, uint64_t row_count, uint32_t* out) {
    if (!tables) return set_err(MH_E_INVALID, "null table set");
    return eval_values_rows(ctx, ts, tables, tapes, n, as, row_first, row_count, out,
                            "mh_eval_values_tables", false);
}

int32_t mh_eval_values_jobs(mh_ctx* ctx, const mh_values_job* jobs, uint32_t n_jobs) {
    // everything below up to use_device() is host-only: a refused list has queued nothing
    if (!ctx) return set_err(MH_E_INVALID, "mh_eval_values_jobs: null ctx");
    if (n_jobs == 0) return MH_OK;
    if (n_jobs > MH_VALUES_JOBS_MAX)
        return set_err(MH_E_INVALID, "mh_eval_values_jobs: " + std::to_string(n_jobs) +
                                         " jobs, more than MH_VALUES_JOBS_MAX (" +
                                         std::to_string(MH_VALUES_JOBS_MAX) + "): chunk the list");
    if (!jobs) return set_err(MH_E_INVALID, "mh_eval_values_jobs: null job list");
    const auto job_err = [](uint32_t i, int32_t code, const std::string& what) {
        return set_err(code, "mh_eval_values_jobs: job " + std::to_string(i) + ": " + what);
    };
    std::vector<mh::values::JobShape> shapes(n_jobs);
    std::vector<std::vector<uint32_t>> variants(n_jobs);
    uint64_t slots = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_values_job& j = jobs[i];
        if (int32_t r = check_run_args(ctx, j.ts, 0, 0, j.as, j.row, 1, MH_MODE_COUNT_ALL))
            return job_err(i, r, g_err);
        if (j.tables) {
            if (int32_t r = check_tables(ctx, j.ts, j.tables)) return job_err(i, r, g_err);
        }
        if (j.n == 0) continue;
        if (!j.tapes || !j.out) return job_err(i, MH_E_INVALID, "null tapes / out");
        variants[i].resize(j.n);
        for (uint32_t k = 0; k < j.n; ++k) {
            if (j.tapes[k] >= j.ts->n_tapes) return job_err(i, MH_E_INVALID, "tape id out of bounds");
            const mh_tape_info& ti = j.ts->info[j.tapes[k]];
            if (!j.tables && (ti.features & F_TABLE))
                return job_err(i, MH_E_UNSUPPORTED,
                               "tape " + std::to_string(j.tapes[k]) +
                                   " holds a table lookup (MH_OP_LOOKUP) and the job has no tables");
            const uint32_t v = mh::variant_of(ti.n_regs, ti.features);
            if (!mh::variant_fits(v, j.as->stride)) {
                (void)refuse_capacity(j.as->stride);
                return job_err(i, MH_E_UNSUPPORTED, g_err);
            }
            variants[i][k] = v;
        }
        shapes[i].ids = j.tapes;
        shapes[i].variants = variants[i].data();
        shapes[i].n = j.n;
        slots += j.n;
    }
    if (slots == 0) return MH_OK;
    if (slots * 8 >= (1ull << 31))
        return set_err(MH_E_INVALID, "mh_eval_values_jobs: values of 2^31 words or more in one call");
    const mh::values::Plan plan = mh::values::plan(shapes.data(), n_jobs);
    // the upload block: segments' KParams | block table | sorted ids
    const auto align = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_seg = 0;
    const size_t o_blk = align(o_seg + plan.segments.size() * sizeof(mh::KParams));
    const size_t o_ids = align(o_blk + plan.blocks.size() * sizeof(mh::batch::BlockEntry));
    const size_t up_bytes = align(o_ids + plan.ids.size() * sizeof(uint32_t));
    const size_t val_bytes = (size_t)slots * 8 * sizeof(uint32_t);
    if (int32_t r = use_device(ctx)) return r;
    if (int32_t r = ctx_batch_bufs(ctx, up_bytes)) return r;
    void* dval_v = nullptr;
    void* hval_v = nullptr;
    MH_HIP(ctx_dbuf(ctx, val_bytes, &dval_v));
    MH_HIP(ctx_hbuf(ctx, val_bytes, &hval_v));
    uint32_t* const dval = static_cast<uint32_t*>(dval_v);
    const uint32_t* const hval = static_cast<const uint32_t*>(hval_v);
    char* const hb = static_cast<char*>(ctx->h_batch);
    char* const db = static_cast<char*>(ctx->d_batch);
    const uint32_t* const d_ids = reinterpret_cast<const uint32_t*>(db + o_ids);
    mh::KParams* h_seg = reinterpret_cast<mh::KParams*>(hb + o_seg);
    for (size_t si = 0; si < plan.segments.size(); ++si) {
        const mh::values::Segment& sg = plan.segments[si];
        const mh_values_job& j = jobs[sg.job];
        // values mode over one row: the count-mode bookkeeping (first_hit / hit_count) has no
        // reader, and sieve_body skips a null array
        mh::KParams p = make_params(j.ts, 0, j.as, j.row, 1, 0, MH_MODE_COUNT_ALL);
        p.tables = j.tables ? j.tables->d : nullptr;
        p.tape_ids = d_ids + sg.first;
        p.n_ids = sg.n_ids;
        p.values_out = dval + 8 * (size_t)sg.first;
        h_seg[si] = p;
    }
    if (int32_t r = batch_spill(ctx, plan, h_seg, [&](const mh::values::Segment& sg) {
            return std::make_pair(jobs[sg.job].ts, plan.ids.data() + sg.first);
        }))
        return r;
    std::memcpy(hb + o_blk, plan.blocks.data(), plan.blocks.size() * sizeof(mh::batch::BlockEntry));
    std::memcpy(hb + o_ids, plan.ids.data(), plan.ids.size() * sizeof(uint32_t));
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(db, hb, up_bytes, hipMemcpyHostToDevice, s);
    const mh::batch::BlockEntry* d_blk = reinterpret_cast<const mh::batch::BlockEntry*>(db + o_blk);
    uint32_t launches = 0;
    for (const auto& l : plan.launches)
        if (e == hipSuccess) {
            e = mh::launch_sieve_batch(reinterpret_cast<const mh::KParams*>(db + o_seg),
                                       d_blk + l.first, l.count, l.variant, s);
            ++launches;
        }
    if (e == hipSuccess) e = hipMemcpyAsync(hval_v, dval, val_bytes, hipMemcpyDeviceToHost, s);
    // the staging area is read by the queued copy: wait even after an error
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess)
        return set_err(MH_E_DEVICE, std::string("mh_eval_values_jobs: ") + hipGetErrorString(e));
    for (uint32_t i = 0; i < n_jobs; ++i)
        for (uint32_t q = plan.job_first[i]; q < plan.job_first[i + 1]; ++q)
            std::memcpy(jobs[i].out + 8 * (size_t)plan.pos[q], hval + 8 * (size_t)q,
                        8 * sizeof(uint32_t));
    ctx->eval_launches += launches;
    return MH_OK;
}

}  // extern "C"

// mh_eval_values_many (tables == null: one row, tapes with lookups refused),
// mh_eval_values_tables and mh_eval_values (`single`: its one tape): out[(i * 8 + k) * row_count + r]
static int32_t eval_values_rows(mh_ctx* ctx, const mh_tapeset* ts, const mh_tables* tables,
                                const uint32_t* tapes, uint32_t n, const mh_assign* as,
                                uint64_t row, uint64_t row_count, uint32_t* out,
                                const char* who, bool single) {
    if (int32_t r = check_run_args(ctx, ts, 0, 0, as, row, row_count, MH_MODE_COUNT_ALL)) return r;
    if (!tables) {
        if (int32_t r = refuse_tables(ts)) return r;
    } else {
        if (int32_t r = check_tables(ctx, ts, tables)) return r;
    }
    if (n == 0 || row_count == 0) return MH_OK;
    if (!tapes || !out) return set_err(MH_E_INVALID, "null tapes / out");
    if (!single && (uint64_t)n * 8 * row_count >= (1ull << 31))
        return set_err(MH_E_INVALID, "values of 2^31 words or more in one call");
    uint32_t top = 0;
    std::vector<uint32_t> variants(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (tapes[i] >= ts->n_tapes) return set_err(MH_E_INVALID, "tape id out of bounds");
        top = std::max(top, tapes[i]);
        variants[i] = mh::variant_of(ts->info[tapes[i]].n_regs, ts->info[tapes[i]].features);
    }
    if (int32_t r = use_device(ctx)) return r;
    // one launch of the production sieve kernel in values mode per variant: the list sorted by
    // (variant, tape id, position) as one job of the batched planner (values_plan.h: the kernel's
    // chunk formation needs the ids of a launch ascending; a repeated id is evaluated again; the
    // caller's order comes back through sorted.pos), its segments as the buckets of the launch
    // planner.  The launches queue on one stream; the spilling tapes' has one region
    const mh::values::JobShape shape{tapes, variants.data(), n};
    mh::values::Plan sorted = mh::values::plan(&shape, 1);
    mh::Buckets ids;
    for (const mh::values::Segment& sg : sorted.segments)
        std::fill(ids.off + sg.variant + 1, ids.off + mh::kNumVariants + 1, sg.first + sg.n_ids);
    ids.ids = std::move(sorted.ids);
    mh::SpillPlan spill;
    const mh::LaunchPlan plan =
        mh::plan_launches(ids, 0, ts->n_tapes, row_count, false, false, as->stride,
                          ts->spills.data(), spill, mh::sieve_launch_waves);
    if (plan.misfit >= 0) return refuse_capacity(as->stride);
    if (int32_t r = spill_reserve(ctx, spill.words)) return r;
    // device block: values [n][8][rows], ids [n], first_hit / hit_count [top + 1] each (scratch:
    // the kernel's count-mode bookkeeping, indexed by tape id)
    const size_t nv = (size_t)8 * n * row_count;  // value words
    const size_t n_words = nv + n + 4 * ((size_t)top + 1) + 2 + (nv & 1);
    // the ctx's grow-only result buffer (stream-ordered after any earlier use of it)
    void* dv = nullptr;
    MH_HIP(ctx_dbuf(ctx, n_words * sizeof(uint32_t), &dv));
    uint32_t* d = static_cast<uint32_t*>(dv);
    uint32_t* d_ids = d + nv;
    uint32_t* d_res = d_ids + n + (((nv + n) & 1) ? 1 : 0);  // 8-byte aligned
    hipError_t e = hipMemcpyAsync(d_ids, ids.ids.data(), n * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(d_res, 0xFF, 2 * ((size_t)top + 1) * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(d_res + 2 * ((size_t)top + 1), 0, 2 * ((size_t)top + 1) * sizeof(uint32_t),
                           ctx->stream);
    for (uint32_t k = 0; k < plan.n && e == hipSuccess; ++k) {
        const mh::Launch& l = plan.launches[k];
        mh::KParams p = make_params(ts, 0, as, row, row_count, 0, MH_MODE_COUNT_ALL);
        p.tables = tables ? tables->d : nullptr;
        p.tape_ids = d_ids + l.first;
        p.n_ids = l.count;
        p.first_hit = reinterpret_cast<unsigned long long*>(d_res);
        p.hit_count = reinterpret_cast<unsigned long long*>(d_res + 2 * ((size_t)top + 1));
        p.values_out = d + 8 * (size_t)l.first * row_count;
        bind_spill(p, ctx, l);
        e = mh::launch_sieve(p, l.variant, ctx->stream);
    }
    std::vector<uint32_t> vals(nv);
    if (e == hipSuccess)
        e = hipMemcpyAsync(vals.data(), d, vals.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess)
        return set_err(MH_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    for (uint32_t i = 0; i < n; ++i)
        std::memcpy(out + 8 * (size_t)sorted.pos[i] * row_count,
                    vals.data() + 8 * (size_t)i * row_count, 8 * row_count * sizeof(uint32_t));
    if (!single) ctx->eval_launches += plan.n;  // the list entry points' counter
    return MH_OK;
}

extern "C" {

int32_t mh_ctx_eval_launches(const mh_ctx* ctx, uint64_t* launches) {
    if (!ctx || !launches) return set_err(MH_E_INVALID, "null argument");
    *launches = ctx->eval_launches;
    return MH_OK;
}

int32_t mh_tapes_jit(mh_tapeset* ts, uint32_t flags, uint32_t max_vgpr) {
    if (!ts) return set_err(MH_E_INVALID, "null tapeset");
    if (ts->has_jit) return set_err(MH_E_INVALID, "tapeset already has native code");
    if (int32_t r = refuse_tables(ts)) return r;
    if (int32_t r = use_device(ts->ctx)) return r;
    const auto t0 = std::chrono::steady_clock::now();
    mh::jit::Options opt;
    opt.max_vgpr = max_vgpr ? max_vgpr : 128;
    opt.short_circuit = (flags & MH_JIT_FULL_EVAL) == 0;
    if (const char* e = std::getenv("MH_JIT_SC")) opt.short_circuit = opt.short_circuit && atoi(e) != 0;
    // gfx950 has 256 architectural VGPRs per wave (an allocation above it would only fail later,
    // in the assembler)
    if (opt.max_vgpr > 256 || opt.max_vgpr < 96) return set_err(MH_E_INVALID, "max_vgpr outside 96..256");
    // build threads = code objects per occupancy class = launches per run: 4 (MI355X, config 5,
    // profiles/r02y: 16 objects 3.195e11 evals/s, 4 3.222e11, 1 3.226e11 -- each launch drains
    // its tail before the next starts; 4 keeps the emission and assembly parallel)
    const uint32_t threads = mh::jit::default_threads();
    std::vector<mh::jit::Built> built;
    mh::jit::BuildStats stats;
    std::string err;
    bool ok;
    try {
        ok = mh::jit::build_tapeset(ts->h_nodes.data(), ts->h_offs.data(), ts->n_tapes,
                                    ts->h_consts.data(), (uint32_t)(ts->h_consts.size() / 8),
                                    ts->n_vars, (flags & MH_JIT_VALUES) != 0, opt, threads, built,
                                    stats, err);
    } catch (const std::bad_alloc&) {
        return set_err(MH_E_NOMEM, "host allocation during JIT build");
    }
    if (!ok) return set_err(MH_E_UNSUPPORTED, "JIT: " + err);
    const uint64_t code_id = mh::jit::code_id(built);
    std::vector<mh_tapeset::JitMod> mods;
    mods.reserve(built.size());
    auto unload = [&]() {
        for (auto& j : mods) {
            if (j.mod) (void)hipModuleUnload(j.mod);
            if (j.vmod) (void)hipModuleUnload(j.vmod);
        }
    };
    uint32_t maxv = 0;
    for (auto& b : built) {
        if (b.hsaco.empty()) continue;
        mods.emplace_back();
        mh_tapeset::JitMod& j = mods.back();
        j.n_groups = b.n_groups;
        j.image.swap(b.hsaco);
        j.vimage.swap(b.hsaco_values);
        hipError_t e = hipModuleLoadData(&j.mod, j.image.data());
        if (e == hipSuccess) e = hipModuleGetFunction(&j.fn, j.mod, "mh_jit");
        if (e == hipSuccess && !j.vimage.empty()) {
            e = hipModuleLoadData(&j.vmod, j.vimage.data());
            if (e == hipSuccess) e = hipModuleGetFunction(&j.vfn, j.vmod, "mh_jit");
        }
        if (e != hipSuccess) {
            unload();
            return set_err(MH_E_DEVICE, std::string("JIT module load: ") + hipGetErrorString(e));
        }
        maxv = std::max(maxv, b.max_vgpr);
    }
    // the interpreter's buckets without the jitted tapes
    mh::Buckets rest = mh::Buckets::build(
        ts->n_tapes, 0,
        [&](uint32_t t) { return mh::variant_of(ts->info[t].n_regs, ts->info[t].features); },
        [&](uint32_t t) { return !stats.jitted[t]; });
    uint32_t* d_rest = nullptr;
    hipError_t e = hipMalloc(&d_rest, std::max<size_t>(1, rest.ids.size()) * sizeof(uint32_t));
    if (e == hipSuccess && !rest.ids.empty())
        e = hipMemcpy(d_rest, rest.ids.data(), rest.ids.size() * sizeof(uint32_t),
                      hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d_rest) (void)hipFree(d_rest);
        unload();
        return set_err(MH_E_DEVICE, std::string("JIT bucket upload: ") + hipGetErrorString(e));
    }
    ts->jit = std::move(mods);
    ts->jitted = stats.jitted;
    ts->rest = std::move(rest);
    ts->d_rest = d_rest;
    ts->has_jit = true;
    ts->code_id = code_id;
    mh_jit_info& ji = ts->jinfo;
    ji = mh_jit_info{};
    for (uint8_t x : stats.jitted) ji.n_jitted += x;
    for (const auto& j : ts->jit) ji.n_groups += j.n_groups;
    ji.n_modules = (uint32_t)ts->jit.size();
    ji.max_vgpr = maxv;
    ji.code_bytes = stats.code_bytes;
    ji.valu_static = stats.valu_static;
    ji.valu_wide_static = stats.valu_wide_static;
    ji.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MH_OK;
}

int32_t mh_tapes_jit_code_id(const mh_tapeset* ts, uint64_t* out) {
    if (!ts || !out) return set_err(MH_E_INVALID, "null argument");
    if (!ts->has_jit) return set_err(MH_E_INVALID, "no native code (mh_tapes_jit first)");
    *out = ts->code_id;
    return MH_OK;
}

int32_t mh_jit_code_id(const mh_node* nodes, const uint64_t* tape_offsets, uint32_t n_tapes,
                       const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                       uint32_t flags, uint32_t max_vgpr, uint64_t* out) {
    if (!out || (n_tapes && (!nodes || !tape_offsets)) || (n_consts && !consts))
        return set_err(MH_E_INVALID, "null argument");
    // the same validation mh_tapes_compile gives a tape set (the JIT reads only checked IR)
    try {
        std::vector<uint32_t> dconsts, w;
        mh::ConstIndex dindex;
        for (uint32_t t = 0; t < n_tapes; ++t) {
            const uint64_t b = tape_offsets[t], e = tape_offsets[t + 1];
            if (e <= b) return set_err(MH_E_INVALID, "tape " + std::to_string(t) + " is empty");
            mh::CompiledTape ct;
            std::string err;
            w.clear();
            const int32_t r = mh::compile_tape(nodes + b, (size_t)(e - b), consts, n_consts,
                                               n_vars, dconsts, dindex, w, ct, err);
            if (r != MH_OK) return set_err(r, "tape " + std::to_string(t) + ": " + err);
        }
    } catch (const std::bad_alloc&) {
        return set_err(MH_E_NOMEM, "host allocation during validation");
    }
    mh::jit::Options opt;
    opt.max_vgpr = max_vgpr ? max_vgpr : 128;
    if (opt.max_vgpr > 256 || opt.max_vgpr < 96) return set_err(MH_E_INVALID, "max_vgpr outside 96..256");
    opt.short_circuit = (flags & MH_JIT_FULL_EVAL) == 0;
    if (const char* e = std::getenv("MH_JIT_SC")) opt.short_circuit = opt.short_circuit && atoi(e) != 0;
    opt.assemble = false;
    std::vector<mh::jit::Built> built;
    mh::jit::BuildStats stats;
    std::string err;
    try {
        if (!mh::jit::build_tapeset(nodes, tape_offsets, n_tapes, consts, n_consts, n_vars, false,
                                    opt, mh::jit::default_threads(), built, stats, err))
            return set_err(MH_E_UNSUPPORTED, "JIT: " + err);
    } catch (const std::bad_alloc&) {
        return set_err(MH_E_NOMEM, "host allocation during JIT build");
    }
    *out = mh::jit::code_id(built);
    return MH_OK;
}

int32_t mh_tapes_jit_info(const mh_tapeset* ts, mh_jit_info* out) {
    if (!ts || !out) return set_err(MH_E_INVALID, "null argument");
    *out = ts->jinfo;
    return MH_OK;
}

int32_t mh_tapes_jitted(const mh_tapeset* ts, uint8_t* out, uint32_t n_tapes) {
    if (!ts || (!out && n_tapes)) return set_err(MH_E_INVALID, "null argument");
    if (n_tapes > ts->n_tapes) return set_err(MH_E_INVALID, "n_tapes exceeds the tape set");
    for (uint32_t t = 0; t < n_tapes; ++t) out[t] = ts->has_jit ? ts->jitted[t] : 0;
    return MH_OK;
}

int32_t mh_jit_eval_all(mh_ctx* ctx, const mh_tapeset* ts, const mh_assign* as,
                        uint64_t row_first, uint64_t row_count, uint32_t* out) {
    if (int32_t r = check_run_args(ctx, ts, 0, ts ? ts->n_tapes : 0, as, row_first, row_count,
                                   MH_MODE_COUNT_ALL))
        return r;
    if (int32_t r = refuse_tables(ts)) return r;
    if (!ts->has_jit) return set_err(MH_E_INVALID, "no native code (mh_tapes_jit first)");
    for (const auto& j : ts->jit)
        if (j.n_groups && !j.vfn) return set_err(MH_E_INVALID, "built without MH_JIT_VALUES");
    if (!out && row_count) return set_err(MH_E_INVALID, "null out");
    if (row_count == 0) return MH_OK;
    if (int32_t r = use_device(ctx)) return r;
    const size_t n = (size_t)ts->n_tapes * 8 * row_count;
    uint32_t* d = nullptr;
    MH_HIP(hipMalloc(&d, n * sizeof(uint32_t)));
    hipError_t e = hipMemcpy(d, out, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    int32_t r = MH_OK;
    if (e == hipSuccess)
        r = launch_jit(ctx, ts, as, row_first, row_count, 0, MH_MODE_COUNT_ALL, nullptr, nullptr, d);
    if (e == hipSuccess && r == MH_OK) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && r == MH_OK) e = hipMemcpy(out, d, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (r != MH_OK) return r;
    if (e != hipSuccess) return set_err(MH_E_DEVICE, std::string("mh_jit_eval_all: ") + hipGetErrorString(e));
    return MH_OK;
}

int32_t mh_comm_unique_id(uint8_t* out) {
    if (!out) return set_err(MH_E_INVALID, "null out");
    const Rccl* r = rccl();
    if (!r) return set_err(MH_E_UNSUPPORTED, "RCCL (librccl.so) not loadable");
    ncclUniqueId id;
    const ncclResult_t e = r->get_unique_id(&id);
    if (e != ncclSuccess)
        return set_err(MH_E_DEVICE, std::string("ncclGetUniqueId: ") +
                                        (r->error_string ? r->error_string(e) : "error"));
    static_assert(sizeof(id) == MH_COMM_ID_BYTES, "RCCL unique id size");
    std::memcpy(out, &id, sizeof(id));
    return MH_OK;
}

int32_t mh_comm_init(mh_ctx* ctx, const uint8_t* unique_id, int32_t rank, int32_t world) {
    if (!ctx || !unique_id) return set_err(MH_E_INVALID, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return set_err(MH_E_INVALID, "bad rank / world");
    if (ctx->comm) return set_err(MH_E_INVALID, "ctx already has a communicator");
    const Rccl* r = rccl();
    if (!r) return set_err(MH_E_UNSUPPORTED, "RCCL (librccl.so) not loadable");
    if (int32_t rc = use_device(ctx)) return rc;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const ncclResult_t e = r->comm_init_rank(&ctx->comm, world, id, rank);
    if (e != ncclSuccess) {
        ctx->comm = nullptr;
        return set_err(MH_E_DEVICE, std::string("ncclCommInitRank: ") +
                                        (r->error_string ? r->error_string(e) : "error"));
    }
    ctx->rank = rank;
    ctx->world = world;
    return MH_OK;
}

int32_t mh_comm_allreduce_results(mh_ctx* ctx, uint64_t* d_first_hit, uint64_t* d_hit_count,
                                  uint32_t n) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    if (!ctx->comm) return set_err(MH_E_INVALID, "no communicator (mh_comm_init)");
    const Rccl* r = rccl();
    if (int32_t rc = use_device(ctx)) return rc;
    // the one exchange of a sharded run: smallest witness index (NO_HIT = UINT64_MAX is the
    // identity of MIN) and summed hit counts, in place on the ctx stream
    ncclResult_t e = ncclSuccess;
    if (d_first_hit && n)
        e = r->all_reduce(d_first_hit, d_first_hit, n, ncclUint64, ncclMin, ctx->comm, ctx->stream);
    if (e == ncclSuccess && d_hit_count && n)
        e = r->all_reduce(d_hit_count, d_hit_count, n, ncclUint64, ncclSum, ctx->comm, ctx->stream);
    if (e != ncclSuccess)
        return set_err(MH_E_DEVICE, std::string("ncclAllReduce: ") +
                                        (r->error_string ? r->error_string(e) : "error"));
    return MH_OK;
}

int32_t mh_comm_destroy(mh_ctx* ctx) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    if (ctx->comm && rccl()) (void)rccl()->comm_destroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->rank = 0;
    ctx->world = 1;
    return MH_OK;
}

int32_t mh_microbench_issue(mh_ctx* ctx, uint32_t kind, uint32_t waves_per_simd,
                            double* lane_ops_per_s) {
    if (!ctx || !lane_ops_per_s || kind >= MH_MB_NUM_KINDS || waves_per_simd == 0 ||
        waves_per_simd > 8)
        return set_err(MH_E_INVALID, "bad argument");
    if (int32_t r = use_device(ctx)) return r;
    // 256 CUs x 4 SIMDs; a 256-thread workgroup is 4 waves, one per SIMD of its CU
    const uint32_t blocks = 256u * waves_per_simd, iters = 8192;
    hipEvent_t e0, e1;
    MH_HIP(hipEventCreate(&e0));
    MH_HIP(hipEventCreate(&e1));
    MH_HIP(mh::launch_microbench(kind, 64, blocks, ctx->scratch, ctx->stream));  // warm-up
    MH_HIP(hipEventRecord(e0, ctx->stream));
    MH_HIP(mh::launch_microbench(kind, iters, blocks, ctx->scratch, ctx->stream));
    MH_HIP(hipEventRecord(e1, ctx->stream));
    MH_HIP(hipEventSynchronize(e1));
    float ms = 0;
    MH_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    // 32 wave-instructions of the measured kind per iteration (kind 7: 32 readlanes + 1 SALU)
    const double lanes = (double)blocks * 256.0;
    *lane_ops_per_s = lanes * iters * 32.0 / (ms * 1e-3);
    return MH_OK;
}

int32_t mh_microbench_valu(mh_ctx* ctx, uint32_t kind, double* ops_per_s) {
    // round-1 entry point: kind 0 add/addc chains, 1 v_mad_u64_u32, 2 v_add_u32 (no carry),
    // each at 8 waves per SIMD
    if (kind > 2) return set_err(MH_E_INVALID, "bad argument");
    return mh_microbench_issue(ctx, kind, 8, ops_per_s);
}

int32_t mh_ctx_enable_timing(mh_ctx* ctx, int32_t enable) {
    if (!ctx) return set_err(MH_E_INVALID, "null ctx");
    ctx->timing = enable != 0;
    return MH_OK;
}

int32_t mh_ctx_kernel_time(mh_ctx* ctx, double* total_ms, uint64_t* launches) {
    if (!ctx || !total_ms || !launches) return set_err(MH_E_INVALID, "null argument");
    if (int32_t r = use_device(ctx)) return r;
    double sum = 0.0;
    hipError_t err = hipSuccess;
    for (auto& sp : ctx->spans) {
        float ms = 0.f;
        if (err == hipSuccess) err = hipEventSynchronize(sp.second);
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, sp.first, sp.second);
        sum += ms;
        (void)hipEventDestroy(sp.first);
        (void)hipEventDestroy(sp.second);
    }
    *launches = ctx->spans.size();
    ctx->spans.clear();
    *total_ms = sum;
    if (err != hipSuccess)
        return set_err(MH_E_DEVICE, std::string("kernel timing: ") + hipGetErrorString(err));
    return MH_OK;
}

// ---- repair of near-miss rows (include/mythril_hip.h; kernels in repair.hip) -------------------
struct mh_repair {
    mh_ctx* ctx = nullptr;
    uint32_t max_conj = 0, max_rows = 0, max_elites = 0;
    unsigned long long* d_masks = nullptr;  // [conjunct][wave of the scored run]
    size_t mask_words = 0;
    uint32_t* d_fail = nullptr;             // [max_rows]
    mh_elite* d_elites = nullptr;           // [max_elites]
    uint32_t* d_plan = nullptr;             // mutate: set_conj | conj_col_off | conj_cols (grow-only)
    size_t plan_words = 0;
    std::vector<uint32_t> h_plan;
    // the last score and select
    bool scored = false, selected = false;
    uint32_t n_conj = 0, row_first = 0, row_count = 0;
    uint64_t stride = 0;
    std::vector<mh_elite> elites;
};

int32_t mh_repair_create(mh_ctx* ctx, uint32_t max_conjuncts, uint32_t max_rows,
                         uint32_t max_elites, mh_repair** out) {
    if (!ctx || !out) return set_err(MH_E_INVALID, "null argument");
    *out = nullptr;
    if (max_conjuncts < 1 || max_conjuncts > 4096 || max_rows < 1 || max_rows > 65536 ||
        max_elites < 1 || max_elites > 256)
        return set_err(MH_E_INVALID, "mh_repair_create: sizes outside 1..4096 conjuncts, "
                                     "1..65536 rows, 1..256 elites");
    if (int32_t r = use_device(ctx)) return r;
    mh_repair* r = new (std::nothrow) mh_repair();
    if (!r) return set_err(MH_E_NOMEM, "repair allocation");
    r->ctx = ctx;
    ++ctx->children;
    r->max_conj = max_conjuncts;
    r->max_rows = max_rows;
    r->max_elites = max_elites;
    // a run's mask stride is its waves, rounded up to whole workgroups (at most 16 waves each)
    r->mask_words = (size_t)max_conjuncts * (max_rows / 64 + 16);
    hipError_t e = hipMalloc(&r->d_masks, r->mask_words * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&r->d_fail, (size_t)max_rows * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&r->d_elites, (size_t)max_elites * sizeof(mh_elite));
    if (e != hipSuccess) {
        mh_repair_destroy(r);
        return set_err(MH_E_NOMEM, std::string("repair buffers: ") + hipGetErrorString(e));
    }
    *out = r;
    return MH_OK;
}

int32_t mh_repair_destroy(mh_repair* r) {
    if (!r) return MH_OK;
    settle(r->ctx);
    (void)hipSetDevice(r->ctx->device);
    if (r->d_masks) (void)hipFree(r->d_masks);
    if (r->d_fail) (void)hipFree(r->d_fail);
    if (r->d_elites) (void)hipFree(r->d_elites);
    if (r->d_plan) (void)hipFree(r->d_plan);
    mh_ctx* ctx = r->ctx;
    delete r;
    ctx_unref(ctx);
    return MH_OK;
}

int32_t mh_repair_score(mh_repair* r, const mh_tapeset* ts, uint32_t tape_first,
                        uint32_t tape_count, const mh_assign* as, uint64_t row_first,
                        uint64_t row_count, uint32_t* fail_count_out) {
    if (!r) return set_err(MH_E_INVALID, "null handle");
    mh_ctx* ctx = r->ctx;
    if (int32_t rc = check_run_args(ctx, ts, tape_first, tape_count, as, row_first, row_count,
                                    MH_MODE_COUNT_ALL))
        return rc;
    if (int32_t rc = refuse_tables(ts)) return rc;
    if (tape_count < 1 || tape_count > r->max_conj)
        return set_err(MH_E_INVALID, "mh_repair_score: conjunct count outside 1..max_conjuncts");
    if (row_count < 1 || row_count > r->max_rows || row_first + row_count > (1ull << 32))
        return set_err(MH_E_INVALID, "mh_repair_score: row count outside 1..max_rows");
    const uint64_t stride = mh::sieve_mask_stride(row_count);
    if (stride * 64 < row_count || (uint64_t)tape_count * stride > r->mask_words)
        return set_err(MH_E_INVALID, "mh_repair_score: the run's masks exceed the handle's buffer");
    if (int32_t rc = use_device(ctx)) return rc;
    mh::KParams p = make_params(ts, tape_first, as, row_first, row_count, 0, MH_MODE_COUNT_ALL);
    p.masks = r->d_masks;
    p.mask_base = tape_first;
    p.mask_stride = stride;
    // a masks-mode launch per kernel-variant bucket of the conjunct tapes, refused before a launch
    mh::SpillPlan spill;
    const mh::LaunchPlan plan =
        mh::plan_launches(ts->all, tape_first, tape_count, row_count, false, true, p.capacity,
                          ts->spills.data(), spill, mh::sieve_launch_waves);
    if (plan.misfit >= 0) return refuse_capacity(p.capacity);
    if (int32_t rc = spill_reserve(ctx, spill.words)) return rc;
    r->scored = r->selected = false;
    MH_HIP(span_begin(ctx));
    for (uint32_t k = 0; k < plan.n; ++k) {
        mh::KParams q = p;
        q.tape_ids = ts->d_all + plan.launches[k].first;
        q.n_ids = plan.launches[k].count;
        bind_spill(q, ctx, plan.launches[k]);
        MH_HIP(mh::launch_sieve(q, plan.launches[k].variant, ctx->stream));
    }
    MH_HIP(mh::launch_fail_count(r->d_masks, stride, tape_count, (uint32_t)row_count, r->d_fail,
                                 ctx->stream));
    MH_HIP(span_end(ctx));
    r->n_conj = tape_count;
    r->row_first = (uint32_t)row_first;
    r->row_count = (uint32_t)row_count;
    r->stride = stride;
    r->scored = true;
    if (fail_count_out) {
        MH_HIP(hipMemcpyAsync(fail_count_out, r->d_fail, row_count * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, ctx->stream));
        MH_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MH_OK;
}

int32_t mh_repair_select(mh_repair* r, uint32_t k, uint64_t seed, mh_elite* out, uint32_t* n_out) {
    if (!r || !out || !n_out) return set_err(MH_E_INVALID, "null argument");
    *n_out = 0;
    if (!r->scored) return set_err(MH_E_INVALID, "mh_repair_select: nothing scored");
    if (k < 1 || k > r->max_elites)
        return set_err(MH_E_INVALID, "mh_repair_select: k outside 1..max_elites");
    mh_ctx* ctx = r->ctx;
    if (int32_t rc = use_device(ctx)) return rc;
    const uint32_t n = std::min(k, r->row_count);
    r->selected = false;
    MH_HIP(span_begin(ctx));
    MH_HIP(mh::launch_select(r->d_masks, r->stride, r->n_conj, r->d_fail, r->row_first,
                             r->row_count, n, seed, r->d_elites, ctx->stream));
    MH_HIP(span_end(ctx));
    r->elites.assign(n, mh_elite{});
    MH_HIP(hipMemcpyAsync(r->elites.data(), r->d_elites, n * sizeof(mh_elite),
                          hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(hipStreamSynchronize(ctx->stream));
    std::copy(r->elites.begin(), r->elites.end(), out);
    *n_out = n;
    r->selected = true;
    return MH_OK;
}

int32_t mh_repair_mutate(mh_repair* r, const mh_assign* src, mh_assign* dst, const mh_guide* guide,
                         const uint32_t* set_conj, const uint32_t* conj_col_off,
                         const uint32_t* conj_cols, uint32_t n_conjuncts, uint32_t per,
                         uint32_t flags, uint64_t seed, uint64_t global_base) {
    if (!r || !src || !dst || !guide || !conj_col_off || (guide->n_sets && !set_conj))
        return set_err(MH_E_INVALID, "null argument");
    mh_ctx* ctx = r->ctx;
    if (src->ctx != ctx || dst->ctx != ctx) return set_err(MH_E_INVALID, "handles of another ctx");
    if (dst == src) return set_err(MH_E_INVALID, "mh_repair_mutate: dst is src");
    if (!r->selected) return set_err(MH_E_INVALID, "mh_repair_mutate: no elites selected");
    if (src->n_vars != dst->n_vars)
        return set_err(MH_E_INVALID, "mh_repair_mutate: buffers of different column counts");
    if (flags & ~MH_MUTATE_REDRAW) return set_err(MH_E_INVALID, "mh_repair_mutate: bad flags");
    const uint32_t n_el = (uint32_t)r->elites.size();
    if (per < 1 || (uint64_t)n_el * per > dst->capacity || (uint64_t)n_el * per > (1ull << 31))
        return set_err(MH_E_INVALID, "mh_repair_mutate: children exceed dst's capacity");
    if (n_conjuncts < 1 || n_conjuncts > r->max_conj)
        return set_err(MH_E_INVALID, "mh_repair_mutate: conjunct count outside 1..max_conjuncts");
    // every index the kernel follows is checked here: it trusts them
    for (const mh_elite& e : r->elites)
        if (e.row >= src->capacity || (e.pick != MH_NO_CONJUNCT && e.pick >= n_conjuncts))
            return set_err(MH_E_INVALID, "mh_repair_mutate: the elites are not of this src / plan");
    if (conj_col_off[0] != 0) return set_err(MH_E_INVALID, "mh_repair_mutate: conj_col_off[0] != 0");
    for (uint32_t t = 0; t < n_conjuncts; ++t)
        if (conj_col_off[t + 1] < conj_col_off[t])
            return set_err(MH_E_INVALID, "mh_repair_mutate: conj_col_off not monotone");
    const uint32_t n_cc = conj_col_off[n_conjuncts];
    if (n_cc && !conj_cols) return set_err(MH_E_INVALID, "mh_repair_mutate: null conj_cols");
    for (uint32_t q = 0; q < n_cc; ++q)
        if (conj_cols[q] >= guide->n_cols)
            return set_err(MH_E_INVALID, "mh_repair_mutate: conjunct column outside the guide");
    for (uint32_t j = 0; j < guide->n_sets; ++j)
        if (set_conj[j] != MH_NO_CONJUNCT && set_conj[j] >= n_conjuncts)
            return set_err(MH_E_INVALID, "mh_repair_mutate: set tag outside the plan");
    mh::KGuide k;
    if (int32_t rc = stage_guide(dst, guide, &k)) return rc;  // checks the guide; uses the device
    const size_t o_tag = 0, o_off = o_tag + guide->n_sets, o_cols = o_off + n_conjuncts + 1,
                 words = o_cols + n_cc;
    r->h_plan.assign(words, 0);
    if (guide->n_sets) std::copy(set_conj, set_conj + guide->n_sets, r->h_plan.begin() + o_tag);
    std::copy(conj_col_off, conj_col_off + n_conjuncts + 1, r->h_plan.begin() + o_off);
    if (n_cc) std::copy(conj_cols, conj_cols + n_cc, r->h_plan.begin() + o_cols);
    if (words > r->plan_words) {
        if (r->d_plan) MH_HIP(hipFree(r->d_plan));
        r->d_plan = nullptr;
        r->plan_words = 0;
        const size_t grow = std::max<size_t>({words, 2 * r->plan_words, (size_t)1 << 12});
        MH_HIP(hipMalloc(&r->d_plan, grow * sizeof(uint32_t)));
        r->plan_words = grow;
    }
    MH_HIP(hipMemcpyAsync(r->d_plan, r->h_plan.data(), words * sizeof(uint32_t),
                          hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(span_begin(ctx));
    MH_HIP(mh::launch_mutate(src->d, src->stride, dst->d, dst->stride, dst->n_vars, r->d_elites,
                             n_el, per, flags, seed, global_base, k, r->d_plan + o_tag,
                             r->d_plan + o_off, r->d_plan + o_cols, ctx->stream));
    MH_HIP(span_end(ctx));
    MH_HIP(hipStreamSynchronize(ctx->stream));  // h_plan is pageable: done with it on return
    return MH_OK;
}

// ---- hit listing and the scatter (include/mythril_hip.h; kernels in hits.hip) -------------------
namespace {

// mh_run_hits' arguments, checked without a device call.  k and the row count come before any
// handle is read.
int32_t check_hits_args(const mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first,
                        uint32_t tape_count, const mh_assign* as, uint64_t row_first,
                        uint64_t row_count, uint32_t k, const uint64_t* hits, const uint32_t* n_hits,
                        uint32_t n_cols, const uint32_t* rows_out, const char* who) {
    const std::string w = std::string(who) + ": ";
    if (!ctx || !ts || !as) return set_err(MH_E_INVALID, w + "null handle (ctx, ts or as)");
    if (k < 1 || k > MH_HITS_MAX)
        return set_err(MH_E_INVALID, w + "k = " + std::to_string(k) + " outside 1..MH_HITS_MAX");
    if (row_count < 1 || row_count > MH_HITS_MAX_ROWS)
        return set_err(MH_E_INVALID, w + "row_count = " + std::to_string(row_count) +
                                         " outside 1..MH_HITS_MAX_ROWS");
    if (!hits || !n_hits) return set_err(MH_E_INVALID, w + "null hits or n_hits");
    if (int32_t r = check_run_args(ctx, ts, tape_first, tape_count, as, row_first, row_count,
                                   MH_MODE_COUNT_ALL))
        return r;
    if (n_cols > as->n_vars)
        return set_err(MH_E_INVALID, w + "n_cols beyond the buffer's columns");
    if (n_cols && !rows_out) return set_err(MH_E_INVALID, w + "rows_out null with n_cols > 0");
    return refuse_tables(ts);
}

// mh_assign_scatter's arguments, checked without a device call.  The order of `cols` comes before
// the handle is read.
int32_t check_scatter_args(const mh_assign* as, uint64_t first, uint32_t n_rows,
                           const uint32_t* cols, uint32_t n_cols, const uint32_t* values,
                           const char* who) {
    const std::string w = std::string(who) + ": ";
    if (!as) return set_err(MH_E_INVALID, w + "null handle (as)");
    if (n_rows && n_cols && (!cols || !values)) return set_err(MH_E_INVALID, w + "null cols or values");
    if (n_rows && cols)
        for (uint32_t c = 1; c < n_cols; ++c)
            if (cols[c] <= cols[c - 1])
                return set_err(MH_E_INVALID, w + "cols not strictly ascending");
    if (n_rows && n_cols && cols[n_cols - 1] >= as->n_vars)
        return set_err(MH_E_INVALID, w + "cols beyond the buffer's columns");
    if (first > as->capacity || n_rows > as->capacity - first)
        return set_err(MH_E_INVALID, w + "rows first + n_rows beyond the buffer's capacity");
    return MH_OK;
}

// A checked scatter queued on the ctx stream: cols | values through the buffer's pinned staging.
int32_t scatter_queue(mh_assign* as, uint64_t first, uint32_t n_rows, const uint32_t* cols,
                      uint32_t n_cols, const uint32_t* values) {
    if (n_rows == 0 || n_cols == 0) return MH_OK;
    if (int32_t r = use_device(as->ctx)) return r;
    const size_t n_val = (size_t)n_rows * n_cols * 8;
    const size_t bytes = (n_cols + n_val) * sizeof(uint32_t);
    if (as->scatter_pending) {  // the last scatter's copy still reads the staging area
        MH_HIP(hipEventSynchronize(as->scattered));
        as->scatter_pending = false;
    }
    if (bytes > as->d_scatter_bytes) {
        // a queued scatter kernel may still read the old device block
        MH_HIP(hipStreamSynchronize(as->ctx->stream));
        MH_HIP(grow_buf(&as->d_scatter, &as->d_scatter_bytes, bytes, 1 << 14, false));
    }
    MH_HIP(grow_buf(&as->h_scatter, &as->h_scatter_bytes, bytes, 1 << 14, true));
    if (!as->scattered) MH_HIP(hipEventCreateWithFlags(&as->scattered, hipEventDisableTiming));
    std::memcpy(as->h_scatter, cols, n_cols * sizeof(uint32_t));
    std::memcpy(as->h_scatter + n_cols, values, n_val * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(as->d_scatter, as->h_scatter, bytes, hipMemcpyHostToDevice,
                          as->ctx->stream));
    MH_HIP(hipEventRecord(as->scattered, as->ctx->stream));
    as->scatter_pending = true;
    MH_HIP(mh::launch_scatter(as->d, as->stride, first, n_rows, as->d_scatter, n_cols,
                              as->d_scatter + n_cols, as->ctx->stream));
    return MH_OK;
}

// A hit-listing run, planned: everything that can refuse it or has to allocate happens in
// hits_plan, before anything of the call is queued; hits_submit queues and waits.
struct HitsPlan {
    mh::LaunchPlan plan;
    uint64_t stride = 0;  // mask words per tape
    size_t n = 0;         // max(tape_count, 1)
    size_t o_count = 0, o_n = 0, o_rows = 0, bytes = 0;  // the result block: hits | counts | n | rows
    void *d = nullptr, *h = nullptr;
};

int32_t hits_plan(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first, uint32_t tape_count,
                  const mh_assign* as, uint64_t row_count, uint32_t k, uint32_t n_cols,
                  HitsPlan* hp) {
    hp->stride = mh::sieve_mask_stride(row_count);
    mh::SpillPlan spill;
    hp->plan = mh::plan_launches(ts->all, tape_first, tape_count, row_count, false, true,
                                 as->stride, ts->spills.data(), spill, mh::sieve_launch_waves);
    if (hp->plan.misfit >= 0) return refuse_capacity(as->stride);
    if (int32_t r = use_device(ctx)) return r;
    if (int32_t r = spill_reserve(ctx, spill.words)) return r;
    hp->n = std::max<uint32_t>(tape_count, 1);
    hp->o_count = hp->n * k * sizeof(uint64_t);
    hp->o_n = hp->o_count + hp->n * sizeof(uint64_t);
    hp->o_rows = hp->o_n + (hp->n * sizeof(uint32_t) + 7) / 8 * 8;
    hp->bytes = hp->o_rows + (size_t)tape_count * k * n_cols * 8 * sizeof(uint32_t);
    // grow-only buffers: a call ends with a stream sync, so nothing queued uses the old blocks
    MH_HIP(grow_buf(&ctx->d_hit_masks, &ctx->hit_masks_bytes,
                    (size_t)hp->n * hp->stride * sizeof(unsigned long long), 1 << 16, false));
    MH_HIP(ctx_dbuf(ctx, hp->bytes, &hp->d));
    MH_HIP(ctx_hbuf(ctx, hp->bytes, &hp->h));
    return MH_OK;
}

int32_t hits_submit(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first, uint32_t tape_count,
                    const mh_assign* as, uint64_t row_first, uint64_t row_count,
                    uint64_t index_base, uint32_t k, const HitsPlan& hp, uint64_t* hits,
                    uint32_t* n_hits, uint64_t* hit_count, uint32_t n_cols, uint32_t* rows_out) {
    if (tape_count == 0) return MH_OK;
    char* d = static_cast<char*>(hp.d);
    const char* h = static_cast<const char*>(hp.h);
    uint64_t* d_hits = reinterpret_cast<uint64_t*>(d);
    mh::KParams p = make_params(ts, tape_first, as, row_first, row_count, index_base,
                                MH_MODE_COUNT_ALL);
    p.masks = ctx->d_hit_masks;
    p.mask_base = tape_first;
    p.mask_stride = hp.stride;
    MH_HIP(span_begin(ctx));
    for (uint32_t i = 0; i < hp.plan.n; ++i) {
        mh::KParams q = p;
        q.tape_ids = ts->d_all + hp.plan.launches[i].first;
        q.n_ids = hp.plan.launches[i].count;
        bind_spill(q, ctx, hp.plan.launches[i]);
        MH_HIP(mh::launch_sieve(q, hp.plan.launches[i].variant, ctx->stream));
    }
    MH_HIP(mh::launch_hits_select(ctx->d_hit_masks, hp.stride, tape_count, (uint32_t)row_count,
                                  index_base + row_first, k, d_hits,
                                  reinterpret_cast<uint32_t*>(d + hp.o_n),
                                  reinterpret_cast<uint64_t*>(d + hp.o_count), ctx->stream));
    MH_HIP(mh::launch_hits_rows(as->d, as->stride, d_hits, tape_count, k, index_base, n_cols,
                                reinterpret_cast<uint32_t*>(d + hp.o_rows), ctx->stream));
    MH_HIP(span_end(ctx));
    // lists, counts and rows in one copy into pinned memory
    MH_HIP(hipMemcpyAsync(hp.h, hp.d, hp.bytes, hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(hits, h, (size_t)tape_count * k * sizeof(uint64_t));
    if (hit_count) std::memcpy(hit_count, h + hp.o_count, tape_count * sizeof(uint64_t));
    std::memcpy(n_hits, h + hp.o_n, tape_count * sizeof(uint32_t));
    if (n_cols) std::memcpy(rows_out, h + hp.o_rows, hp.bytes - hp.o_rows);
    return MH_OK;
}

}  // namespace

int32_t mh_run_hits(mh_ctx* ctx, const mh_tapeset* ts, uint32_t tape_first, uint32_t tape_count,
                    const mh_assign* as, uint64_t row_first, uint64_t row_count,
                    uint64_t index_base, uint32_t k, uint64_t* hits, uint32_t* n_hits,
                    uint64_t* hit_count, uint32_t n_cols, uint32_t* rows_out) {
    if (int32_t r = check_hits_args(ctx, ts, tape_first, tape_count, as, row_first, row_count, k,
                                    hits, n_hits, n_cols, rows_out, "mh_run_hits"))
        return r;
    HitsPlan hp;
    if (int32_t r = hits_plan(ctx, ts, tape_first, tape_count, as, row_count, k, n_cols, &hp))
        return r;
    return hits_submit(ctx, ts, tape_first, tape_count, as, row_first, row_count, index_base, k, hp,
                       hits, n_hits, hit_count, n_cols, rows_out);
}

int32_t mh_assign_scatter(mh_assign* as, uint64_t first, uint32_t n_rows, const uint32_t* cols,
                          uint32_t n_cols, const uint32_t* values) {
    if (int32_t r = check_scatter_args(as, first, n_rows, cols, n_cols, values, "mh_assign_scatter"))
        return r;
    return scatter_queue(as, first, n_rows, cols, n_cols, values);
}

int32_t mh_query_round_hits(mh_ctx* ctx, const mh_tapeset* ts, mh_assign* as, const mh_guide* guide,
                            uint64_t seed, uint64_t global_base, uint64_t count,
                            uint32_t tape_first, uint32_t tape_count, const mh_spares* spares,
                            uint32_t k, uint64_t* hits, uint32_t* n_hits, uint64_t* hit_count,
                            uint32_t n_cols, uint32_t* rows_out) {
    if (int32_t r = check_hits_args(ctx, ts, tape_first, tape_count, as, 0, count, k, hits, n_hits,
                                    n_cols, rows_out, "mh_query_round_hits"))
        return r;
    if (!guide) return set_err(MH_E_INVALID, "mh_query_round_hits: null guide");
    if (spares) {
        if (spares->n_rows > count)
            return set_err(MH_E_INVALID, "mh_query_round_hits: spares->n_rows beyond count");
        if (int32_t r = check_scatter_args(as, 0, spares->n_rows, spares->cols, spares->n_cols,
                                           spares->values, "mh_query_round_hits: spares"))
            return r;
    }
    GuideLayout L;
    if (int32_t r = check_guide(as, guide, &L)) return r;
    HitsPlan hp;
    if (int32_t r = hits_plan(ctx, ts, tape_first, tape_count, as, count, k, n_cols, &hp)) return r;
    // the generator, the scatter, the run and the copy queue back to back: one host sync
    if (int32_t r = mh_assign_generate_guided(as, seed, global_base, 0, count, guide)) return r;
    if (spares)
        if (int32_t r = scatter_queue(as, 0, spares->n_rows, spares->cols, spares->n_cols,
                                      spares->values))
            return r;
    return hits_submit(ctx, ts, tape_first, tape_count, as, 0, count, global_base, k, hp, hits,
                       n_hits, hit_count, n_cols, rows_out);
}

int32_t mh_query_round_hits_many(mh_ctx* ctx, const mh_round_hits_job* jobs, uint32_t n_jobs) {
    // everything below up to use_device() is host-only: a refused batch has queued nothing
    const std::string who = "mh_query_round_hits_many: ";
    if (!ctx) return set_err(MH_E_INVALID, who + "null ctx");
    if (n_jobs == 0) return MH_OK;
    if (n_jobs > MH_ROUND_MANY_MAX)
        return set_err(MH_E_INVALID, who + std::to_string(n_jobs) +
                                         " jobs, more than MH_ROUND_MANY_MAX (" +
                                         std::to_string(MH_ROUND_MANY_MAX) + "): chunk the list");
    if (!jobs) return set_err(MH_E_INVALID, who + "null job list");
    const auto job_err = [&](uint32_t i, int32_t code, const std::string& what) {
        return set_err(code, who + "job " + std::to_string(i) + ": " + what);
    };
    // k and the row count of every job come before any handle is read
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_hits_job& j = jobs[i];
        if (j.k < 1 || j.k > MH_HITS_MAX)
            return job_err(i, MH_E_INVALID, "k = " + std::to_string(j.k) +
                                                " outside 1..MH_HITS_MAX");
        if (j.count == 0)
            return job_err(i, MH_E_INVALID, "count = 0 outside 1..MH_HITS_MAX_ROWS");
    }
    struct JobPlan {
        GuideLayout L;
        mh::Buckets::Range in[mh::kNumVariants];  // the job's tapes per bucket
        size_t guide_off = 0, sp_off = 0;         // bytes of the device block
        uint64_t mask_off = 0, mask_stride = 0;   // words of the ctx's hit masks
        size_t o_hits = 0, o_count = 0, o_n = 0, o_rows = 0, rows_bytes = 0;  // result block
    };
    std::vector<JobPlan> jp(n_jobs);
    std::vector<mh::batch::JobShape> shapes(n_jobs);
    // the kernels' prefix tables: select | rows | scatter workgroups, n_jobs + 1 entries each
    std::vector<uint32_t> prefix(3 * ((size_t)n_jobs + 1), 0);
    uint32_t* const pre_sel = prefix.data();
    uint32_t* const pre_rows = pre_sel + n_jobs + 1;
    uint32_t* const pre_sc = pre_rows + n_jobs + 1;
    size_t res_bytes = 0;
    uint64_t mask_words = 0;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_hits_job& j = jobs[i];
        JobPlan& p = jp[i];
        if (!j.ts || !j.as || !j.guide) return job_err(i, MH_E_INVALID, "null handle");
        if (j.ts->ctx != ctx || j.as->ctx != ctx)
            return job_err(i, MH_E_INVALID, "handles of another ctx");
        if (!j.hits || !j.n_hits) return job_err(i, MH_E_INVALID, "null hits or n_hits");
        for (uint32_t q = 0; q < i; ++q)
            if (jobs[q].as == j.as)
                return job_err(i, MH_E_INVALID, "shares its assignment buffer with job " +
                                                    std::to_string(q));
        if (j.count > mh::batch::kMaxRows)
            return job_err(i, MH_E_UNSUPPORTED, std::to_string(j.count) + " rows, more than " +
                                                    std::to_string(mh::batch::kMaxRows));
        if (j.count > j.as->capacity)
            return job_err(i, MH_E_UNSUPPORTED, std::to_string(j.count) +
                                                    " rows, more than the buffer's capacity");
        if (int32_t r = check_run_args(ctx, j.ts, j.tape_first, j.tape_count, j.as, 0, j.count,
                                       MH_MODE_COUNT_ALL))
            return job_err(i, r, g_err);
        if (j.n_cols > j.as->n_vars)
            return job_err(i, MH_E_INVALID, "n_cols beyond the buffer's columns");
        if (j.n_cols && !j.rows_out)
            return job_err(i, MH_E_INVALID, "rows_out null with n_cols > 0");
        if (int32_t r = refuse_tables(j.ts)) return job_err(i, r, g_err);
        uint32_t sp_rows = 0, sp_cols = 0;
        if (j.spares) {
            if (j.spares->n_rows > j.count)
                return job_err(i, MH_E_INVALID, "spares->n_rows beyond count");
            if (int32_t r = check_scatter_args(j.as, 0, j.spares->n_rows, j.spares->cols,
                                               j.spares->n_cols, j.spares->values, "spares"))
                return job_err(i, r, g_err);
            if (j.spares->n_rows && j.spares->n_cols) {
                sp_rows = j.spares->n_rows;
                sp_cols = j.spares->n_cols;
            }
        }
        if (int32_t r = check_guide(j.as, j.guide, &p.L)) return job_err(i, r, g_err);
        // the job's tapes per interpreter bucket: whole tapes (ts->all), never split parts
        mh::batch::JobShape& sh = shapes[i];
        sh.count = j.count;
        sh.whole = j.tape_first == 0 && j.tape_count == j.ts->n_tapes;
        sh.gen_n_cols = p.L.nc;
        sh.gen_span_words = (uint32_t)(p.L.o_eval - p.L.o_prob);
        for (uint32_t v = 0; v < mh::kNumVariants; ++v) {
            p.in[v] = j.ts->all.range(v, j.tape_first, j.tape_count);
            sh.n_ids[v] = p.in[v].count;
        }
        // the job's slices of the masks and of the result block (mh_run_hits' layout per job)
        const size_t tc = j.tape_count;
        p.mask_stride = mh::sieve_mask_stride(j.count);
        p.mask_off = mask_words;
        mask_words += tc * p.mask_stride;
        p.o_hits = res_bytes;
        p.o_count = p.o_hits + tc * j.k * sizeof(uint64_t);
        p.o_n = p.o_count + tc * sizeof(uint64_t);
        p.o_rows = p.o_n + (tc * sizeof(uint32_t) + 7) / 8 * 8;
        p.rows_bytes = tc * j.k * j.n_cols * 8 * sizeof(uint32_t);
        res_bytes = p.o_rows + p.rows_bytes;
        if (res_bytes > MH_ROUND_HITS_MANY_MAX_BYTES)
            return job_err(i, MH_E_UNSUPPORTED,
                           "the batch's lists and rows up to this job take " +
                               std::to_string(res_bytes) +
                               " bytes, more than MH_ROUND_HITS_MANY_MAX_BYTES (" +
                               std::to_string(MH_ROUND_HITS_MANY_MAX_BYTES) +
                               "): chunk the list or ask for fewer hits");
        pre_sel[i + 1] = pre_sel[i] + j.tape_count;
        pre_rows[i + 1] = pre_rows[i] + (j.n_cols ? j.tape_count * j.k : 0);
        pre_sc[i + 1] = pre_sc[i] + mh::scatter_blocks(sp_rows, sp_cols);
    }
    const mh::batch::Plan plan = mh::batch::plan(shapes.data(), n_jobs);
    // a launch's variant serves every segment in it: each must fit that segment's buffer
    for (const auto& l : plan.launches)
        for (uint32_t b = l.first; b < l.first + l.count; ++b) {
            const uint32_t job = plan.segments[plan.blocks[b].seg].job;
            if (!mh::variant_fits(l.variant, jobs[job].as->stride)) {
                (void)refuse_capacity(jobs[job].as->stride);
                return job_err(job, MH_E_UNSUPPORTED, g_err);
            }
        }
    // the device block: segments' KParams | GenJob[] | HitsJob[] | prefix tables | block tables |
    // guides | spares (cols, values per job)
    const auto align = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_seg = 0;
    const size_t o_gen = align(o_seg + plan.segments.size() * sizeof(mh::KParams));
    const size_t o_hj = align(o_gen + n_jobs * sizeof(mh::GenJob));
    const size_t o_pre = align(o_hj + n_jobs * sizeof(mh::HitsJob));
    const size_t o_blk = align(o_pre + prefix.size() * sizeof(uint32_t));
    const size_t o_gblk = align(o_blk + plan.blocks.size() * sizeof(mh::batch::BlockEntry));
    size_t up_bytes = align(o_gblk + plan.gen_blocks.size() * sizeof(mh::batch::GenEntry));
    for (uint32_t i = 0; i < n_jobs; ++i) {
        jp[i].guide_off = up_bytes;
        up_bytes = align(up_bytes + jp[i].L.words * sizeof(uint32_t));
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        jp[i].sp_off = up_bytes;
        if (pre_sc[i + 1] != pre_sc[i]) {
            const mh_spares& sp = *jobs[i].spares;
            up_bytes = align(up_bytes +
                             (sp.n_cols + (size_t)sp.n_rows * sp.n_cols * 8) * sizeof(uint32_t));
        }
    }
    if (int32_t r = use_device(ctx)) return r;
    if (int32_t r = ctx_batch_bufs(ctx, up_bytes)) return r;
    // grow-only buffers: a call ends with a stream sync, so nothing queued uses the old blocks
    MH_HIP(grow_buf(&ctx->d_hit_masks, &ctx->hit_masks_bytes,
                    (size_t)std::max<uint64_t>(mask_words, 1) * sizeof(unsigned long long), 1 << 16,
                    false));
    void* dres_v = nullptr;
    void* hres_v = nullptr;
    MH_HIP(ctx_dbuf(ctx, std::max<size_t>(res_bytes, 8), &dres_v));
    MH_HIP(ctx_hbuf(ctx, std::max<size_t>(res_bytes, 8), &hres_v));
    char* const dres = static_cast<char*>(dres_v);
    const char* const hres = static_cast<const char*>(hres_v);
    char* const hb = static_cast<char*>(ctx->h_batch);
    char* const db = static_cast<char*>(ctx->d_batch);
    // fill the staging area
    mh::GenJob* h_gen = reinterpret_cast<mh::GenJob*>(hb + o_gen);
    mh::HitsJob* h_hj = reinterpret_cast<mh::HitsJob*>(hb + o_hj);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_hits_job& j = jobs[i];
        const JobPlan& p = jp[i];
        pack_guide(j.guide, p.L, reinterpret_cast<uint32_t*>(hb + p.guide_off));
        mh::GenJob g{};
        g.assign = j.as->d;
        g.stride = j.as->stride;
        g.count = j.count;
        g.seed = j.seed;
        g.base = j.global_base;
        g.g = guide_at(p.L, reinterpret_cast<const uint32_t*>(db + p.guide_off));
        h_gen[i] = g;
        mh::HitsJob h{};
        h.masks = ctx->d_hit_masks + p.mask_off;
        h.mask_stride = p.mask_stride;
        h.index0 = j.global_base;
        h.assign = j.as->d;
        h.stride = j.as->stride;
        h.o_hits = p.o_hits;
        h.o_hit_count = p.o_count;
        h.o_n_hits = p.o_n;
        h.o_rows = p.o_rows;
        h.row_count = (uint32_t)j.count;
        h.k = j.k;
        h.n_cols = j.n_cols;
        if (pre_sc[i + 1] != pre_sc[i]) {
            const mh_spares& sp = *j.spares;
            uint32_t* w = reinterpret_cast<uint32_t*>(hb + p.sp_off);
            std::memcpy(w, sp.cols, sp.n_cols * sizeof(uint32_t));
            std::memcpy(w + sp.n_cols, sp.values,
                        (size_t)sp.n_rows * sp.n_cols * 8 * sizeof(uint32_t));
            h.sp_cols = reinterpret_cast<const uint32_t*>(db + p.sp_off);
            h.sp_values = h.sp_cols + sp.n_cols;
            h.sp_rows = sp.n_rows;
            h.sp_n_cols = sp.n_cols;
        }
        h_hj[i] = h;
    }
    // every segment in masks mode, writing into its job's slice of the hit masks
    mh::KParams* h_seg = reinterpret_cast<mh::KParams*>(hb + o_seg);
    for (size_t si = 0; si < plan.segments.size(); ++si) {
        const mh::batch::Segment& sg = plan.segments[si];
        const mh_round_hits_job& j = jobs[sg.job];
        mh::KParams p = make_params(j.ts, j.tape_first, j.as, 0, j.count, j.global_base,
                                    MH_MODE_COUNT_ALL);
        p.masks = ctx->d_hit_masks + jp[sg.job].mask_off;
        p.mask_base = j.tape_first;
        p.mask_stride = jp[sg.job].mask_stride;
        p.tape_ids = j.ts->d_all + jp[sg.job].in[sg.first_bucket].first;
        p.n_ids = sg.n_ids;
        h_seg[si] = p;
    }
    if (int32_t r = batch_spill(ctx, plan, h_seg, [&](const mh::batch::Segment& sg) {
            const mh_tapeset* ts = jobs[sg.job].ts;
            return std::make_pair(ts, ts->all.ids.data() + jp[sg.job].in[sg.first_bucket].first);
        }))
        return r;
    std::memcpy(hb + o_pre, prefix.data(), prefix.size() * sizeof(uint32_t));
    if (!plan.blocks.empty())
        std::memcpy(hb + o_blk, plan.blocks.data(),
                    plan.blocks.size() * sizeof(mh::batch::BlockEntry));
    if (!plan.gen_blocks.empty())
        std::memcpy(hb + o_gblk, plan.gen_blocks.data(),
                    plan.gen_blocks.size() * sizeof(mh::batch::GenEntry));
    MH_HIP(span_begin(ctx));  // one span for the whole submission
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(db, hb, up_bytes, hipMemcpyHostToDevice, s);
    const mh::GenJob* d_gen = reinterpret_cast<const mh::GenJob*>(db + o_gen);
    const mh::HitsJob* d_hj = reinterpret_cast<const mh::HitsJob*>(db + o_hj);
    const uint32_t* d_pre = reinterpret_cast<const uint32_t*>(db + o_pre);
    const mh::batch::GenEntry* d_gblk = reinterpret_cast<const mh::batch::GenEntry*>(db + o_gblk);
    const mh::batch::BlockEntry* d_blk = reinterpret_cast<const mh::batch::BlockEntry*>(db + o_blk);
    for (const auto& l : plan.gen_launches)
        if (e == hipSuccess)
            e = mh::launch_generate_guided_batch(d_gen, d_gblk + l.first, l.count, l.form,
                                                 l.lds_bytes, s);
    if (e == hipSuccess)
        e = mh::launch_scatter_batch(d_hj, d_pre + 2 * ((size_t)n_jobs + 1), n_jobs,
                                     pre_sc[n_jobs], s);
    for (const auto& l : plan.launches)
        if (e == hipSuccess)
            e = mh::launch_sieve_batch(reinterpret_cast<const mh::KParams*>(db + o_seg),
                                       d_blk + l.first, l.count, l.variant, s);
    if (e == hipSuccess)
        e = mh::launch_hits_select_batch(d_hj, d_pre, n_jobs, pre_sel[n_jobs], dres, s);
    if (e == hipSuccess)
        e = mh::launch_hits_rows_batch(d_hj, d_pre + n_jobs + 1, n_jobs, pre_rows[n_jobs], dres, s);
    if (e == hipSuccess) e = span_end(ctx);
    if (e == hipSuccess && res_bytes)
        e = hipMemcpyAsync(hres_v, dres, res_bytes, hipMemcpyDeviceToHost, s);
    // the staging area is read by the queued copy: wait even after an error
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_err(MH_E_DEVICE, who + hipGetErrorString(e));
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const mh_round_hits_job& j = jobs[i];
        const JobPlan& p = jp[i];
        const size_t tc = j.tape_count;
        if (!tc) continue;
        std::memcpy(j.hits, hres + p.o_hits, tc * j.k * sizeof(uint64_t));
        if (j.hit_count) std::memcpy(j.hit_count, hres + p.o_count, tc * sizeof(uint64_t));
        std::memcpy(j.n_hits, hres + p.o_n, tc * sizeof(uint32_t));
        if (j.n_cols) std::memcpy(j.rows_out, hres + p.o_rows, p.rows_bytes);
    }
    return MH_OK;
}

}  // extern "C"
