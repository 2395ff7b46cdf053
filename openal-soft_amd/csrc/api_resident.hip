// The resident voice kernel's host side (OALGPU_CTX_RESIDENT; device side and protocol: kernels.hpp ResidentDoor, voice_wave.hip,
// post_wave.hip; the context's part: api_context.hpp ResidentState): who is running and how they are told to leave, the set-up,
// one update's doorbell with its reduction and post-process, the error report, the statistics and the mode's setters.
// (Part of the C-ABI shim: see api.hip.)
#include "api_context.hpp"

// ---- who is running, and how they are told to leave ----
namespace {
std::mutex gResLock;                        // submit / park of every context's resident state
std::vector<oalgpu_context*> gResRunning;
std::atomic<int> gResCount{0};              // gResRunning's size, for the look without the lock (ParkResidentContexts)

// (gResLock held) a launch of `c` is on the main stream and has not been told to leave / it has been, or leaves by itself
void ResidentEnter(oalgpu_context *c)
{
    c->res.running = true;
    gResRunning.push_back(c);
    gResCount.store(int(gResRunning.size()), std::memory_order_relaxed);
}
void ResidentLeave(oalgpu_context *c)
{
    c->res.running = false;
    gResRunning.erase(std::remove(gResRunning.begin(), gResRunning.end(), c), gResRunning.end());
    gResCount.store(int(gResRunning.size()), std::memory_order_relaxed);
}

// (gResLock held) the running launch finishes the updates that have been rung and ends; nothing waits here
void ResidentParkLocked(oalgpu_context *c)
{
    auto &R = c->res;
    if(!R.running) return;
    __atomic_store_n(&R.door->exitSeq[R.launches & 3u], R.next, __ATOMIC_RELEASE);     // (R.launches: the running launch's id)
    __builtin_ia32_sfence();                // (write-combined stores through the BAR leave the core)
    ResidentLeave(c);
    ++R.parks;
    R.shortRuns = (R.next - R.launchBase < R.shortRun) ? R.shortRuns + 1u : 0u;
    if(R.shortRuns >= 3u) { R.shortRuns = 0u; R.cooldown = 192u; }
    const uint32_t e = (R.launches - 1u) % oalgpu_context::ResidentState::kEv;
    R.evLast[e] = R.next;
}

// everything the context has in flight, on its three streams
void ResidentDrain(oalgpu_context *c)
{
    (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->res.reduceStream); (void)hipStreamSynchronize(c->postStream);
}

// spins until `done()`, for five seconds at the most (the clock is read every 1024 spins) -> false: the time ran out
template<typename Done>
bool SpinFiveSeconds(Done done)
{
    using clk = std::chrono::steady_clock;
    const auto deadline = clk::now() + std::chrono::seconds(5);
    uint32_t spins = 0;
    while(!done())
    {
        __builtin_ia32_pause();
        if((++spins & 0x3ffu) == 0 && clk::now() > deadline) return false;
    }
    return true;
}
} // namespace

namespace oalgpu {
// resident voice kernels running on `device` are told to leave (UseDevice, api.hip)
void ParkResidentContexts(int device)
{
    if(gResCount.load(std::memory_order_relaxed) == 0) return;
    std::lock_guard<std::mutex> g(gResLock);
    std::vector<oalgpu_context*> run = gResRunning;
    for(oalgpu_context *c : run) if(c->desc.device == device) ResidentParkLocked(c);
}
} // namespace oalgpu

bool ResidentWanted(const oalgpu_context *c, int post_process)
{
    const auto &R = c->res;
    return R.enabled && !R.failed && WaveKernelHasResident(c->L) && post_process && c->hrtfLoaded && c->directSet && !c->timing && c->cbVoices.empty()
        && c->initPending.empty() && c->carryAccum && !c->comm && !c->pendingMix.active() && c->useWave && c->ownStream && !c->serialOnly
        && c->L.numReal >= 2 && c->L.numSlots == 0 && c->attached.empty();
}

// a parameter block that was waiting for a resident update is applied the launched way (the caller has parked the kernel)
int FlushResidentBlock(oalgpu_context *c)
{
    oalgpu_param_block *b = c->res.pendingBlock;
    if(!b) return OALGPU_OK;
    c->res.pendingBlock = nullptr;
    b->heldBy = nullptr;
    if(int rc = FlushInits(c)) return rc;
    LaunchApplyParams(c->stream, c->L, b->recs.p, b->count);
    HIP_TRY(hipGetLastError());
    return OALGPU_OK;
}

static int ResidentGiveUp(oalgpu_context *c, const std::string &why)
{
    c->res.failed = true;
    return Fail(OALGPU_ERR_HIP, "resident voice kernel: " + why + " (the context launches per update from now on)");
}

// streams, the door, counters, partial sets: once per context, with nothing resident on the device
static int ResidentInit(oalgpu_context *c)
{
    auto &R = c->res;
    if(int rc = UseDevice(c->desc.device)) return rc;
    hipDeviceProp_t prop{};
    HIP_TRY(hipGetDeviceProperties(&prop, c->desc.device));
    // every workgroup of the launch has to be on the machine at once: nothing ever leaves to make room
    R.groupsPerCu = uint32_t(std::max(0, WaveResidentGroupsPerCu(c->L)));
    if(uint64_t{R.groupsPerCu} * uint32_t(prop.multiProcessorCount) < c->L.numGroups)
        return ResidentGiveUp(c, "the device does not hold all of the launch's workgroups at once");
    // the reduce stream between the main stream's priority class (highest) and the post stream's (lowest): a class has its own
    // hardware queues, and a queue the resident kernel sits in never moves
    int prioLeast = 0, prioGreatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prioLeast, &prioGreatest));
    if(prioLeast - prioGreatest < 2) return ResidentGiveUp(c, "fewer than three stream priority classes");
    HIP_TRY(hipStreamCreateWithPriority(&R.reduceStream, hipStreamDefault, (prioLeast + prioGreatest) / 2));
    R.doorInBar = HostStoresReachDevice(c);
    if(R.doorInBar) HIP_TRY(hipExtMallocWithFlags(reinterpret_cast<void**>(&R.door), sizeof(ResidentDoor), hipDeviceMallocFinegrained));
    else HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&R.door), sizeof(ResidentDoor), hipHostMallocDefault));
    std::memset(R.door, 0, sizeof(ResidentDoor));
    for(uint32_t &e : R.door->exitSeq) e = 0x40000000u;
    __builtin_ia32_sfence();
    HIP_TRY(R.counters.alloc(size_t{kRcCount} * 16)); HIP_TRY(R.counters.zero());
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&R.hostFlags), size_t{kRhCount} * 16 * sizeof(uint32_t), hipHostMallocDefault));
    std::memset(R.hostFlags, 0, size_t{kRhCount} * 16 * sizeof(uint32_t));
    R.setFloats = size_t{c->L.numGroups} * (kLine + kHrirLen) * 2;
    HIP_TRY(R.part.alloc(R.setFloats * kResidentSets));
    for(uint32_t k = 0; k < oalgpu_context::ResidentState::kEv; ++k) { HIP_TRY(hipEventCreate(&R.evStart[k])); HIP_TRY(hipEventCreate(&R.evStop[k])); }
    R.firGroups = PostResidentFirGroups();
    R.redGroups = uint32_t((BusFloats(c->L) + 63u) / 64u);
    R.ready = true;
    return OALGPU_OK;
}

// the launches whose events have fired hand over their times
void ResidentCollectTimes(oalgpu_context *c, bool all)
{
    auto &R = c->res;
    for(uint32_t k = 0; k < oalgpu_context::ResidentState::kEv; ++k)
    {
        if(!R.evOpen[k] || (R.running && k == (R.launches - 1u) % oalgpu_context::ResidentState::kEv)) continue;
        if(!all && hipEventQuery(R.evStop[k]) != hipSuccess) { (void)hipGetLastError(); continue; }
        float ms = 0.0f;
        if(hipEventElapsedTime(&ms, R.evStart[k], R.evStop[k]) == hipSuccess)
        {
            R.kernelMs += double(ms); R.kernelUpdates += R.evLast[k] - R.evFirst[k]; ++R.kernelLaunches;
        }
        else (void)hipGetLastError();
        R.evOpen[k] = false;
    }
}

int ResidentCheckError(oalgpu_context *c)
{
    auto &R = c->res;
    if(!R.hostFlags) return OALGPU_OK;
    const uint32_t e = __atomic_load_n(R.hostFlags + 16u * kRhError, __ATOMIC_ACQUIRE);
    if(!e) return OALGPU_OK;
    __atomic_store_n(R.hostFlags + 16u * kRhError, 0u, __ATOMIC_RELEASE);
    static const char *what[4] = {"", "the voice kernel waited 2 s for the host or for its reduction", "a reduction waited 2 s for the voice kernel",
        "a reduction waited 2 s for the post-process"};
    // where everything stood: the counters the kernels wait for, beside what the host expects them to reach
    std::string state;
    {
        ResidentDrain(c);
        uint32_t w[kRcCount * 16] = {};
        uint32_t pa = 0;
        if(hipMemcpy(w, R.counters.p, sizeof(w), hipMemcpyDeviceToHost) == hipSuccess
            && hipMemcpy(&pa, c->postArrived.p, sizeof(pa), hipMemcpyDeviceToHost) == hipSuccess)
        {
            char buf[512];
            std::snprintf(buf, sizeof(buf), " [updates %u, launches %u, groups %u; arrive %u %u %u %u (uses %u %u %u %u), redRead %u redDone %u (per update %u), "
                "postDone %u (posts %u x %u), postArrived %u (epoch %u), started %u (expected %u), progress %u]", R.next, R.launches, c->L.numGroups,
                w[0], w[16], w[32], w[48], R.setUses[0], R.setUses[1], R.setUses[2], R.setUses[3], w[16 * kRcRedRead], w[16 * kRcRedDone], R.redGroups,
                w[16 * kRcPostDone], R.posts, R.firGroups, pa, c->postEpoch, w[16 * kRcStarted], R.startedTotal,
                __atomic_load_n(R.hostFlags + 16u * kRhProgress, __ATOMIC_ACQUIRE));
            state = buf;
            const uint32_t *fi = R.hostFlags + 16u * kRhFault;
            std::snprintf(buf, sizeof(buf), " [the voice workgroup that gave up: update %u, doorbell %u, exit word %u, reduction counter %u of %u, workgroup %u, launch %u, "
                "%u ticks; host: seq %u exit %u %u %u %u]", fi[0], fi[1], fi[2], fi[3], fi[4], fi[5], fi[6], fi[7], R.door->seq, R.door->exitSeq[0], R.door->exitSeq[1],
                R.door->exitSeq[2], R.door->exitSeq[3]);
            if(e == 1) state += buf;
        }
        else (void)hipGetLastError();
    }
    return ResidentGiveUp(c, std::string(e < 4 ? what[e] : "a wait timed out") + state);
}

// One update of a resident context: the doorbell, its reduction (reduce stream) and its post-process (post stream).
// Returns 1 when the update has to go the launched way after all (the caller falls through), 0 when submitted, < 0 on errors.
int ResidentSubmit(oalgpu_context *c, uint32_t samples_to_do)
{
    auto &R = c->res;
    if(!R.ready) { if(int rc = ResidentInit(c)) return R.failed ? 1 : rc; }
    HIP_TRY(hipSetDevice(c->desc.device));
    std::unique_lock<std::mutex> g(gResLock);
    const DeviceLayout &L = c->L;
    // a new launch: prepared here, started BEHIND the update's doorbell (the kernel finds its first update rung when it comes up)
    const bool launchNow = !R.running;
    ResidentArgs a{};
    uint32_t evk = 0;
    bool timed = false;
    if(launchNow)
    {
        // the reduce stream joins whatever the post stream still runs (the bus block and the carried accumulator are theirs too)
        if(c->postPending) HIP_TRY(hipStreamWaitEvent(R.reduceStream, c->lastPostEvent ? c->lastPostEvent : c->evPostDone, 0));
        const uint32_t k = evk = R.launches % oalgpu_context::ResidentState::kEv;
        if(R.evOpen[k]) { HIP_TRY(hipEventSynchronize(R.evStop[k])); ResidentCollectTimes(c, false); }
        timed = R.timeLaunches;           // (events bound to the dispatch cost the launch call ~15 us of host time)
        a.door = R.door; a.counters = R.counters.p; a.hostFlags = R.hostFlags; a.partBase = R.part.p; a.setStride = uint32_t(R.setFloats);
        a.base = R.next; a.endSeq = R.next + R.maxUpdates; a.redPerUpdate = R.redGroups;
        a.startedTarget = R.startedTotal + L.numGroups; a.launchId = R.launches + 1u;
        __atomic_store_n(&R.door->exitSeq[a.launchId & 3u], R.next + 0x40000000u, __ATOMIC_RELEASE);
        __atomic_store_n(&R.door->seq, R.next, __ATOMIC_RELEASE);
        __builtin_ia32_sfence();
    }
    // the host stays at most kResidentDepth updates ahead of the post-process (doorbell slots, queue depth)
    if(!SpinFiveSeconds([&] { return int32_t(R.posts - __atomic_load_n(R.hostFlags + 16u * kRhProgress, __ATOMIC_ACQUIRE)) < int32_t(kResidentDepth); }))
    {
        ResidentParkLocked(c);
        g.unlock();
        ResidentDrain(c);
        if(int rc = ResidentCheckError(c)) return rc;
        return ResidentGiveUp(c, "the post-process made no progress for 5 s");
    }
    if(__atomic_load_n(R.hostFlags + 16u * kRhError, __ATOMIC_RELAXED))
    {
        ResidentParkLocked(c);
        g.unlock();
        ResidentDrain(c);
        return ResidentCheckError(c);
    }
    c->outRingWritten = false;
    // ---- the doorbell: the slot first, then the sequence number
    oalgpu_param_block *b = R.pendingBlock;
    R.pendingBlock = nullptr;
    if(b) b->heldBy = nullptr;
    ResidentSlot &sl = R.door->slot[R.next % kResidentSlots];
    sl.recs = b ? reinterpret_cast<unsigned long long>(b->recs.p) : 0ull;
    sl.map = b ? reinterpret_cast<unsigned long long>(b->voiceToRec.p) : 0ull;
    sl.rows = b ? reinterpret_cast<unsigned long long>(b->rows.p) : 0ull;
    sl.samples = samples_to_do;
    __builtin_ia32_sfence();
    __atomic_store_n(&R.door->seq, R.next + 1u, __ATOMIC_RELEASE);
    __builtin_ia32_sfence();
    if(launchNow)
    {
        const uint32_t k = evk;
        HIP_TRY(LaunchVoiceWaveResident(c->stream, L, a, timed ? R.evStart[k] : nullptr, timed ? R.evStop[k] : nullptr));
        R.evOpen[k] = timed; R.evFirst[k] = R.next; R.evLast[k] = R.next;
        ++R.launches; R.startedTotal = a.startedTarget; R.endSeq = a.endSeq; R.launchBase = R.next;
        // Nothing that waits for this kernel may get onto the machine in front of it: a reduction that polls for workgroups which
        // find no room beside it would wait for ever.  The last workgroup to start says so (a pinned word): the doorbell is rung at
        // once -- the workgroups that are there start on the update -- and the host looks for the word only in front of the first
        // reduction it launches (awaitStarted), which nobody needs before the voices of the update are through.
        R.awaitStarted = a.launchId;
        ResidentEnter(c);
    }
    // ---- the update's reduction and post-process: launches of their own that wait for device counters
    const uint32_t set = R.next % kResidentSets;
    if(R.awaitStarted)
    {
        const uint32_t id = R.awaitStarted;
        R.awaitStarted = 0u;
        if(!SpinFiveSeconds([&] { return __atomic_load_n(R.hostFlags + 16u * kRhResident, __ATOMIC_ACQUIRE) == id; }))
        {   // (it may still start, and the update has been rung: it is told to leave behind that update; the update is lost)
            ++R.next;
            ResidentParkLocked(c);
            g.unlock();
            (void)hipStreamSynchronize(c->stream);
            return ResidentGiveUp(c, "its workgroups did not all start within 5 s");
        }
    }
    if(R.copyPending) { HIP_TRY(hipStreamWaitEvent(R.reduceStream, R.copyPending, 0)); R.copyPending = nullptr; }
    DeviceLayout Lr = L;
    Lr.partHrtf = R.part.p + size_t{set} * R.setFloats;
    LaunchBusReduceResident(R.reduceStream, Lr, CarrySource(c, true), R.counters.p, R.hostFlags, set, (R.setUses[set] + 1u) * L.numGroups,
        R.posts * R.firGroups);
    HIP_TRY(hipGetLastError());
    ++R.setUses[set];
    c->lastPostEvent = c->evPostDone;
    if(int rc = PostDirectHrtfFused(c, c->postStream, samples_to_do, c->limOn ? nullptr : c->evPostDone, true)) return rc;
    if(c->limOn)
    {   // the limiter behind the update's post-process; the next update's reduction (reduce stream) rewrites the lines it limits
        if(int rc = RunLimiter(c, c->postStream, samples_to_do)) return rc;
        HIP_TRY(hipEventRecord(c->evPostDone, c->postStream));
        R.copyPending = c->evPostDone;
    }
    c->postPending = true;
    ++R.next;
    ++c->updatesSubmitted;
    R.evLast[(R.launches - 1u) % oalgpu_context::ResidentState::kEv] = R.next;
    // the launch's own bound: it leaves by itself behind this update; the next one starts a new launch
    if(R.next == R.endSeq) ResidentLeave(c);
    return OALGPU_OK;
}

int oalgpu_resident_stats(oalgpu_context *c, oalgpu_resident_info *out)
{
    if(!c || !out) return Fail(OALGPU_ERR_INVALID, "null argument");
    auto &R = c->res;
    uint32_t w[kRcCount * 16] = {};
    if(R.ready && !R.running)
    {   // the wait counters: a copy on the null stream, with nothing resident on the device
        if(int rc = UseDevice(c->desc.device)) return rc;
        HIP_TRY(hipMemcpy(w, R.counters.p, sizeof(w), hipMemcpyDeviceToHost));
    }
    std::lock_guard<std::mutex> g(gResLock);
    out->enabled = R.enabled ? 1 : 0; out->failed = R.failed ? 1 : 0; out->running = R.running ? 1 : 0;
    out->door_in_device_memory = R.doorInBar ? 1 : 0;
    out->launches = R.launches; out->updates = R.next; out->parks = uint32_t(R.parks);
    out->timed_launches = uint32_t(R.kernelLaunches); out->timed_updates = R.kernelUpdates; out->timed_kernel_ms = R.kernelMs;
    out->max_updates_per_launch = R.maxUpdates; out->pad = 0;
    // (the voice kernel's words: every 128th workgroup keeps them)
    const double tick = 0.01, groups = double(std::max<uint32_t>((c->L.numGroups + 127u) / 128u, 1u));
    out->wait_door_us = w[16 * kRcWaitDoor] * tick / groups; out->wait_reduction_us = w[16 * kRcWaitRed] * tick / groups;
    out->wait_arrival_us = w[16 * kRcWaitArrive] * tick; out->wait_post_us = w[16 * kRcWaitPost] * tick;
    out->wait_reduced_us = w[16 * kRcWaitRedDone] * tick; out->wait_split_us = w[16 * kRcWaitSplit] * tick;
    out->install_us = w[16 * kRcInstall] * tick / groups; out->busy_us = w[16 * kRcBusy] * tick / groups;
    out->top_us = w[16 * kRcTop] * tick / groups;
    return OALGPU_OK;
}

int oalgpu_resident_set_short_run(oalgpu_context *c, uint32_t updates)
{
    if(!c) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(int rc = UseCtx(c)) return rc;
    c->res.shortRun = updates;
    c->res.shortRuns = 0; c->res.cooldown = 0;
    return OALGPU_OK;
}

int oalgpu_resident_set_timing(oalgpu_context *c, int enable)
{
    if(!c) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(int rc = UseCtx(c)) return rc;           // (the running launch ends: the next one carries the events, or no longer does)
    c->res.timeLaunches = enable != 0;
    return OALGPU_OK;
}

int oalgpu_resident_set_max_updates(oalgpu_context *c, uint32_t max_updates)
{
    if(!c || max_updates == 0 || max_updates > 0x10000000u) return Fail(OALGPU_ERR_INVALID, "oalgpu_resident_set_max_updates: 1 .. 2^28");
    if(int rc = UseCtx(c)) return rc;
    c->res.maxUpdates = max_updates;
    return OALGPU_OK;
}
