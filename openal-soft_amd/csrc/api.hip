// C-ABI shim (include/oalgpu.h) over the HIP kernels.  Host logic only: argument checks,
// HBM allocation/upload, parameter preparation that the reference does with libm on its mixer
// thread (resampler state, biquad design), and kernel launches on the context's stream.
// No CPU fallback exists anywhere in this file: without a HIP device every entry point fails.
// This file: context life, the voice kernel's grid rules, the update and its entry points.
// (The rest of the C-ABI: api_resident.hip, api_attach.hip, api_slots.hip, api_comm.hip, api_percall.hip, api_hrtf.hip,
// api_buffers.hip, api_voices.hip, api_output.hip, api_poststage.hip, api_callback.hip; shared: api_context.hpp.)
#include "api_context.hpp"
namespace oalgpu {

thread_local std::string gLastError;

int Fail(int code, const std::string &msg)
{
    gLastError = msg;
    return code;
}

// Every entry point that may allocate, copy synchronously or wait for the device comes through here.  A resident voice kernel
// ends only when its host says so, and anything that synchronises the device (hipFree, a blocking hipMemcpy, the null stream)
// would wait for it for ever: so whoever selects the device first parks the resident kernels on it (they finish the updates
// that have been rung and leave; the next oalgpu_mix_update of such a context launches a new one).
int UseDevice(int device)
{
    int count = 0;
    if(hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return Fail(OALGPU_ERR_NO_DEVICE, "no HIP device available (the product has no CPU path)");
    if(device < 0 || device >= count) return Fail(OALGPU_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    ParkResidentContexts(device);
    return OALGPU_OK;
}

} // namespace oalgpu

// every entry point that enqueues work on a context or reads its state goes through here: the device (which parks a resident
// voice kernel: whatever follows on the main stream then runs behind its end), a parameter block that was waiting for a
// resident update, and the deferred update
int UseCtx(oalgpu_context *c)
{
    if(int rc = UseDevice(c->desc.device)) return rc;
    if(int rc = FlushResidentBlock(c)) return rc;
    return FlushPendingMix(c);
}
// the entry points a resident voice kernel stays through (they touch neither the main stream nor anything that synchronises the device)
int UseCtxResident(oalgpu_context *c)
{
    if(!c->res.running && !c->res.pendingBlock) return UseCtx(c);
    HIP_TRY(hipSetDevice(c->desc.device));
    return OALGPU_OK;
}

// (shared with the other C-ABI translation units: api_context.hpp)

// the voice slot is re-initialised as another kind of source: its callback is not asked any more
void RetireCallbackVoice(oalgpu_context *c, uint32_t voice)
{
    if(voice < c->cbOfVoice.size() && c->cbOfVoice[voice] >= 0)
    {
        auto &cb = c->cbVoices[size_t(c->cbOfVoice[voice])];
        cb.state = OALGPU_VOICE_STOPPED;
        cb.retired = true;                          // buffer slot, device and pinned memory wait for the next callback source
        c->cbOfVoice[voice] = -1;
    }
}

// a callback voice's mStep, wherever parameters pass through the host
void NoteCallbackSteps(oalgpu_context *c, const uint32_t *voices, const oalgpu_voice_params *params, size_t count)
{
    if(c->cbVoices.empty()) return;
    for(size_t i = 0; i < count; ++i)
        if(voices[i] < c->cbOfVoice.size() && c->cbOfVoice[voices[i]] >= 0)
            c->cbVoices[size_t(c->cbOfVoice[voices[i]])].step = params[i].step;
}

int FlushInits(oalgpu_context *c)
{
    if(c->initPending.empty()) return OALGPU_OK;
    const size_t n = c->initPending.size();
    if(int rc = StageRecords(c->stream, c->initDev, c->initPending.data(), n)) return rc;
    LaunchInitVoices(c->stream, c->L, c->initDev.p, uint32_t(n));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->initPending.clear();
    return OALGPU_OK;
}

// the device's compute units (256 on an MI355X, the figure assumed when the query fails)
uint32_t DeviceComputeUnits(int device)
{
    hipDeviceProp_t prop{};
    if(hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) return uint32_t(prop.multiProcessorCount);
    (void)hipGetLastError();
    return 256u;
}

// An EAX reverb instance is ONE workgroup that needs a compute unit's LDS nearly to itself (128 KB: both pipelines' rows,
// csrc/reverb_kernels.hip), and it runs on the post stream beside the NEXT update's voice kernel.  A voice kernel whose grid fills
// the machine exactly (two 78 KB workgroups on every CU) then finds the instances' CUs taken: the workgroups it cannot place wait
// for a second round, and the launch lasts 1.6 times as long (BASELINE configs[3]: 110 -> 174 us in every other update, the
// reverbs 85 -> 170 us in the updates between, profiles/r5/evidence/step_timeline_config4.txt).  With reverbs attached the
// automatic voices-per-workgroup choice therefore leaves the instances their CUs: a few more voices per wavefront, so that the
// grid fits on the CUs that are left -- one round, and the reverbs run beside it undisturbed.
// voice_rows.hip's grid: one workgroup of eight wavefronts per compute unit -- the compute units the attached EAX reverb instances need
// (a whole CU's LDS each, beside the NEXT update's voice kernel, see above) left out --, the voices dealt evenly
static void SetRowsGroups(oalgpu_context *c)
{
    DeviceLayout &L = c->L;
    const uint32_t reverbs = AttachedReverbs(c);
    const uint32_t cus = DeviceComputeUnits(c->desc.device);
    const uint32_t waves = RowsWavesPerGroup();
    uint32_t groups = std::min<uint32_t>(cus > reverbs ? cus - reverbs : 1u, (L.numVoices + waves - 1u) / waves);
    if(c->desc.voices_per_group) groups = (L.numVoices + c->desc.voices_per_group - 1u) / c->desc.voices_per_group;
    groups = std::max<uint32_t>(1u, std::min<uint32_t>(groups, c->groupsAllocated));
    L.rowsVpg = (L.numVoices + groups - 1u) / groups;
    L.numGroups = (L.numVoices + L.rowsVpg - 1u) / L.rowsVpg;
    L.numLineGroups = L.numGroups;
}

int RebalanceWaveGroups(oalgpu_context *c)
{
    if(c->useWave && c->L.rows8)
    {
        const uint32_t before = c->L.rowsVpg;
        DeviceLayout T = c->L;
        SetRowsGroups(c);
        if(c->L.rowsVpg != before)
        {   // (the streams may still run launches of the old grid)
            const DeviceLayout N = c->L;
            c->L = T;
            if(int rc = oalgpu_sync(c)) return rc;
            c->L = N;
        }
        return OALGPU_OK;
    }
    if(!c->useWave || c->desc.voices_per_group != 0u || c->L.wave16) return OALGPU_OK;
    const uint32_t reverbs = AttachedReverbs(c);
    hipDeviceProp_t prop{};
    if(hipGetDeviceProperties(&prop, c->desc.device) != hipSuccess || prop.multiProcessorCount <= 0) { (void)hipGetLastError(); return OALGPU_OK; }
    const uint32_t cus = uint32_t(prop.multiProcessorCount);
    const uint32_t slots = 2u * (cus > reverbs ? cus - reverbs : 1u);          // two voice workgroups per compute unit
    DeviceLayout &L = c->L;
    uint32_t vpw = std::max<uint32_t>(1u, (c->desc.max_voices + 2047u) / 2048u);  // (oalgpu_context_create's rule)
    const uint32_t full = 2u * cus;
    auto groupsOf = [&](uint32_t w) { DeviceLayout T = L; T.waveVoices = w; return WaveKernelGroups(T); };
    // only a grid that was meant to fill the machine in one round is thinned out (smaller scenes leave room anyway)
    if(reverbs && groupsOf(vpw) <= full) { while(groupsOf(vpw) > slots) ++vpw; }
    if(vpw == L.waveVoices) return OALGPU_OK;
    if(int rc = oalgpu_sync(c)) return rc;
    L.waveVoices = vpw;
    L.numGroups = std::max<uint32_t>(1u, WaveKernelGroups(L));       // (never more than the context's buffers were sized for)
    L.numLineGroups = L.numGroups;
    return OALGPU_OK;
}

int oalgpu_context_create(const oalgpu_context_desc *desc, oalgpu_context **out)
{
    if(!desc || !out) return Fail(OALGPU_ERR_INVALID, "null argument");
    *out = nullptr;
    if(desc->max_voices == 0 || desc->num_dry_channels == 0 || desc->num_dry_channels > OALGPU_MAX_OUTPUT_CHANNELS
        || desc->num_aux_sends > OALGPU_MAX_SENDS || desc->wet_channels > OALGPU_MAX_AMBI_CHANNELS
        || (desc->num_aux_sends && (desc->num_slots == 0 || desc->wet_channels == 0)))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_context_create: bad descriptor");
    const uint32_t mixLines = (desc->hrtf ? 0u : desc->num_dry_channels) + desc->num_slots * desc->wet_channels;
    if(mixLines > 32) return Fail(OALGPU_ERR_CAPACITY, "more than 32 mixing lines (dry + wet) are not supported yet");
    if(int rc = UseDevice(desc->device)) return rc;

    auto c = std::make_unique<oalgpu_context>();
    c->desc = *desc;
    c->exact = desc->math_mode == OALGPU_MATH_EXACT;
    // The context's two streams must never share a hardware queue: HIP deals streams of one priority
    // class round-robin onto GPU_MAX_HW_QUEUES (default 4) queues, and a process that created other
    // streams first (torch, RCCL) can leave both on the same one -- the post stream's work then
    // serialises with the voice kernels (measured: 86 instead of 52 us per update).  Each priority
    // class has its own queues, so the main stream takes the highest and the post stream the lowest.
    int prioLeast = 0, prioGreatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prioLeast, &prioGreatest));
    HIP_TRY(hipStreamCreateWithPriority(&c->stream, hipStreamDefault, prioGreatest));
    HIP_TRY(hipEventCreate(&c->evStart)); HIP_TRY(hipEventCreate(&c->evVoice)); HIP_TRY(hipEventCreate(&c->evEnd));
    HIP_TRY(hipStreamCreateWithPriority(&c->postStream, hipStreamDefault, prioLeast));
    std::vector<hipEvent_t*> orderEvents{&c->evVoiceDone[0], &c->evVoiceDone[1], &c->evPostDone};
    for(hipEvent_t &e : c->evReduceDone) orderEvents.push_back(&e);
    for(hipEvent_t *e : orderEvents)
        // ordering between the context's two streams only: no system-scope fence (the default one
        // costs ~3.5 us of cache write-back per record on the stream it sits in -- measured, tools/
        // step_period.py; hosts and peers see the results through oalgpu_sync / stream order as before)
        HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventDisableSystemFence));

    DeviceLayout &L = c->L;
    L.numVoices = desc->max_voices;
    L.numDry = desc->num_dry_channels; L.numReal = desc->num_real_channels;
    L.numSends = desc->num_aux_sends; L.numSlots = desc->num_slots; L.wetChannels = desc->wet_channels;
    L.hrtf = desc->hrtf ? 1u : 0u;
    L.irSize = 0; L.irStride = 8;
    L.mixLines = mixLines;
    c->slots.assign(desc->num_slots, EffectSlot{});
    c->slotOrder.resize(desc->num_slots);
    for(uint32_t i = 0; i < desc->num_slots; ++i) c->slotOrder[i] = i;
    HIP_TRY(c->reverbTicket.alloc(1)); HIP_TRY(c->reverbTicket.zero());
    uint32_t vpg = desc->voices_per_group;
    if(vpg == 0)
    {
        // enough groups to put several workgroups on each of the 256 CUs, but no more partial
        // buses than needed: aim for ~1024 groups, at least 2 voices per group
        vpg = std::max<uint32_t>(2u, (desc->max_voices + 1023u) / 1024u);
    }
    L.voicesPerGroup = vpg;
    L.numGroups = std::max<uint32_t>(1u, (desc->max_voices + vpg - 1u) / vpg);
    L.waveVoices = 0;
    // the HRTF FIR of the wavefront kernel (IrSize <= 64): the matrix pipe in split half precision
    // (FirMfmaH, dev_wave.hpp) unless the host asks for packed fp32 VALU FMAs
    L.firMfma = (desc->flags & OALGPU_CTX_FIR_VALU) ? 0u : 1u;
    c->serialOnly = (desc->flags & OALGPU_CTX_SERIAL) != 0;
    c->res.enabled = (desc->flags & OALGPU_CTX_RESIDENT) != 0 && !(desc->flags & (OALGPU_CTX_PROFILE | OALGPU_CTX_SERIAL));
    c->useWave = WaveKernelApplies(c->exact, L);
    if(c->useWave)
    {
        // one wavefront per voice, 4 wavefronts per workgroup, two workgroups per CU: aim for
        // ~512 workgroups (2048 wavefronts); voices_per_group is then voices per WORKGROUP
        L.waveVoices = desc->voices_per_group ? std::max<uint32_t>(1u, (desc->voices_per_group + 3u) / 4u)
            : std::max<uint32_t>(1u, (desc->max_voices + 2047u) / 2048u);
        L.numGroups = std::max<uint32_t>(1u, WaveKernelGroups(L));
    }
    const TableBlob &blob = Blob();
    HIP_TRY(c->tables.alloc(blob.data.size())); HIP_TRY(c->tables.upload(blob.data.data(), blob.data.size()));
    L.tables = c->tables.p;
    HIP_TRY(c->buffers.alloc(std::max<uint32_t>(desc->max_buffers, 1u))); HIP_TRY(c->buffers.zero());
    L.buffers = c->buffers.p;
    c->buf.reset(desc->max_buffers, desc->max_voices);
    c->cbOfVoice.assign(std::max<uint32_t>(desc->max_voices, 1u), -1);

    const size_t nv = desc->max_voices;
    HIP_TRY(c->ctl.alloc(nv)); HIP_TRY(c->ctl.zero()); L.ctl = c->ctl.p;
    HIP_TRY(c->prev.alloc(nv * kMaxPad)); HIP_TRY(c->prev.zero()); L.prev = c->prev.p;
    HIP_TRY(c->dfilt.alloc(nv * 2)); HIP_TRY(c->dfilt.zero()); L.dfilt = c->dfilt.p;
    HIP_TRY(c->hist.alloc(nv * kHist)); HIP_TRY(c->hist.zero()); L.hist = c->hist.p;
    HIP_TRY(c->gainCur.alloc(nv * L.numDry)); HIP_TRY(c->gainCur.zero()); L.gainCur = c->gainCur.p;
    HIP_TRY(c->gainTgt.alloc(nv * L.numDry)); HIP_TRY(c->gainTgt.zero()); L.gainTgt = c->gainTgt.p;
    HIP_TRY(c->sfilt.alloc(nv * L.numSends * 2)); HIP_TRY(c->sfilt.zero()); L.sfilt = c->sfilt.p;
    HIP_TRY(c->sendCur.alloc(nv * L.numSends * L.wetChannels)); HIP_TRY(c->sendCur.zero()); L.sendCur = c->sendCur.p;
    HIP_TRY(c->sendTgt.alloc(nv * L.numSends * L.wetChannels)); HIP_TRY(c->sendTgt.zero()); L.sendTgt = c->sendTgt.p;
    HIP_TRY(c->ambi.alloc(nv)); HIP_TRY(c->ambi.zero()); L.ambi = c->ambi.p;
    HIP_TRY(c->startDelay.alloc(nv)); HIP_TRY(c->startDelay.zero()); L.startDelay = c->startDelay.p;
    {   // identity ambisonic maps until the host hands over the device's (ACN i, scale 1)
        std::vector<AmbiMapEntry> ident(std::max<size_t>(L.numDry, size_t{L.numSlots} * L.wetChannels) + 1);
        for(size_t i = 0; i < ident.size(); ++i) ident[i] = AmbiMapEntry{uint32_t(i < OALGPU_MAX_AMBI_CHANNELS ? i : 0), 1.0f};
        HIP_TRY(c->dryMap.alloc(L.numDry)); HIP_TRY(c->dryMap.upload(ident.data(), L.numDry));
        HIP_TRY(c->wetMaps.alloc(size_t{L.numSlots} * L.wetChannels));
        for(uint32_t s = 0; s < L.numSlots; ++s)
            HIP_TRY(hipMemcpy(c->wetMaps.p + size_t{s} * L.wetChannels, ident.data(), L.wetChannels * sizeof(AmbiMapEntry), hipMemcpyHostToDevice));
    }
    HIP_TRY(c->queueDone.alloc(nv)); HIP_TRY(c->queueDone.zero()); L.queueDone = c->queueDone.p;
    L.numLineGroups = L.numGroups;
    c->groupsAllocated = L.numGroups;
    if(c->useWave && L.hrtf && L.firMfma && !(desc->flags & OALGPU_CTX_WAVE_PAIRS))
    {   // the voice-per-wavefront form InstallHrtfData may choose (voice_wave16.hip) has a grid of voices / 4, 8 or 16 workgroups: above
        // 8192 voices, or with voices_per_group, more than the two-voices-per-wavefront grid above -- the partial buses fit the larger
        const uint32_t w = Wave16WavesFor(desc->max_voices, DeviceComputeUnits(desc->device));
        c->groupsAllocated = std::max<uint32_t>(c->groupsAllocated, (desc->max_voices + w - 1u) / w);
    }
    L.streams = nullptr; L.lineGains = nullptr; L.lineStride = 0; L.streamsPerVoice = 0;
    L.nfc = nullptr; L.nfcOrders = 0;
    L.hrirs = nullptr;
    for(uint32_t &n : L.chansPerOrder) n = 0;
    L.accLines = 0;
    L.wave16 = 0;                           // (decided when the HRTF data set is known: InstallHrtfData)
    L.rows8 = 0; L.rowsVpg = 0;
    if(c->useWave && !(desc->flags & OALGPU_CTX_STREAM_ROWS))
    {
        L.accLines = WaveKernelAccLines(L);
        // dry lines AND sends, or more lines than the wavefront-per-voice kernel holds in registers: by default
        // the rows stay in LDS -- a wavefront per voice produces, a wavefront per 128-frame slice of every line
        // consumes, the round's filters are jobs dealt to all eight wavefronts (voice_rows.hip); one workgroup per compute unit
        // (SetRowsGroups below).  OALGPU_CTX_STREAM_ROWS keeps the rows in HBM (above); OALGPU_CTX_ROW_SLICES asks for this form by name.
        if(!L.accLines && RowsKernelApplies(L))
            L.rows8 = 1;
    }
    if(c->useWave && (!L.hrtf || L.numSends))
    {   // one partial bus per workgroup, from the wavefronts' line accumulators (accLines) or from stream rows mixed by the
        // voice kernel's tail
        L.lineStride = L.mixLines <= 8 ? 8u : (L.mixLines <= 16 ? 16u : 32u);
        L.streamsPerVoice = 2u + L.numSends;
    }
    if(c->useWave && (!L.hrtf || L.numSends) && !L.accLines && !L.rows8) { if(int rc = AllocStreamRows(c.get())) return rc; }
    const size_t groups = c->groupsAllocated;
    HIP_TRY(c->partLines.alloc(groups * L.mixLines * kLine)); L.partLines = c->partLines.p;
    // the two-stream pipeline of oalgpu_mix_update alternates between two sets of partial buses
    HIP_TRY(c->partLines2.alloc(c->useWave && (L.streams || L.accLines || L.rows8) ? groups * L.mixLines * kLine : 0));
    c->partLinesBuf[0] = c->partLines.p; c->partLinesBuf[1] = c->partLines2.p;
    HIP_TRY(c->partHrtf.alloc(L.hrtf ? groups * (kLine + kHrirLen) * 2 : 0)); L.partHrtf = c->partHrtf.p;
    HIP_TRY(c->partHrtf2.alloc(c->useWave && L.hrtf ? groups * (kLine + kHrirLen) * 2 : 0));
    c->partHrtfBuf[0] = c->partHrtf.p; c->partHrtfBuf[1] = c->partHrtf2.p;
    if(c->useWave && L.hrtf && L.numSends == 0 && (desc->flags & OALGPU_CTX_APPLY_IN_VOICE_KERNEL) && !(desc->flags & OALGPU_CTX_SPAN_ONE))
    {   // a voice launch of such a context may cover up to kSpanMax deferred updates, each with a partial set of its own: sets for two launches in flight
        const size_t setFloats = groups * (kLine + kHrirLen) * 2;
        HIP_TRY(c->partHrtfMore.alloc(setFloats * (oalgpu_context::kPartSets - 2u)));
        for(uint32_t k = 2; k < oalgpu_context::kPartSets; ++k) c->partHrtfBuf[k] = c->partHrtfMore.p + setFloats * (k - 2u);
        c->numSets = oalgpu_context::kPartSets;
    }
    if(desc->flags & OALGPU_CTX_SPAN_ONE) c->launchSpan = 1u;
    HIP_TRY(c->bus.alloc(BusFloats(L))); HIP_TRY(c->bus.zero()); L.bus = c->bus.p;
    if(desc->flags & OALGPU_CTX_PROFILE)
    {
        HIP_TRY(c->phaseTimes.alloc(nv * 16)); HIP_TRY(c->phaseTimes.zero());   // [voice][8] | [wavefront][8]
        c->prof.times = c->phaseTimes.p;
    }
    // HRTF voice filters are sized when the data set is loaded
    L.hrtfOld = nullptr; L.hrtfTgt = nullptr;

    HIP_TRY(c->dSplit.alloc(L.numDry)); HIP_TRY(c->dSplit.zero());
    HIP_TRY(c->dSplit2.alloc(L.numDry)); HIP_TRY(c->dSplit2.zero());
    HIP_TRY(c->carryBuf.alloc(size_t{kLine + kHrirLen} * 2)); HIP_TRY(c->carryBuf.zero());
    HIP_TRY(c->postArrived.alloc(1)); HIP_TRY(c->postArrived.zero());
    HIP_TRY(c->dHfScale.alloc(L.numDry)); HIP_TRY(c->dHfScale.zero());
    HIP_TRY(c->dCoeffs.alloc(size_t{L.numDry} * kHrirLen * 2)); HIP_TRY(c->dCoeffs.zero());
    HIP_TRY(c->dTemp.alloc(size_t{L.numDry} * kLine + (kLine + kHrirLen) * 2));
    if(L.rows8) SetRowsGroups(c.get());
    *out = c.release();
    return OALGPU_OK;
}

void oalgpu_context_destroy(oalgpu_context *ctx)
{
    if(!ctx) return;
    (void)UseDevice(ctx->desc.device);          // (a resident voice kernel is told to leave)
    if(ctx->attachedTo || !ctx->attached.empty()) DetachForDestroy(ctx);
    if(ctx->res.pendingBlock) { ctx->res.pendingBlock->heldBy = nullptr; ctx->res.pendingBlock = nullptr; }
    (void)FlushPendingMix(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    if(ctx->res.reduceStream) (void)hipStreamSynchronize(ctx->res.reduceStream);
    if(ctx->postStream) (void)hipStreamSynchronize(ctx->postStream);
    delete ctx->comm;
    for(auto &cb : ctx->cbVoices)
        for(int k = 0; k < 2; ++k)
        {
            if(cb.pinned[k]) (void)hipHostFree(cb.pinned[k]);
            if(cb.copied[k]) (void)hipEventDestroy(cb.copied[k]);
        }
    delete ctx;
}

// stream rows [voice][streamsPerVoice][1024] and their gain blocks, for the contexts whose voice kernel mixes them in its tail
int AllocStreamRows(oalgpu_context *c)
{
    DeviceLayout &L = c->L;
    const size_t nv = L.numVoices;
    HIP_TRY(c->streams.alloc(nv * L.streamsPerVoice * kLine)); HIP_TRY(c->streams.zero()); L.streams = c->streams.p;
    HIP_TRY(c->lineGains.alloc(nv * L.streamsPerVoice * LineBlockDwords(L.lineStride))); HIP_TRY(c->lineGains.zero());
    L.lineGains = c->lineGains.p;
    return OALGPU_OK;
}

// Where the reduction finds the carried HrtfAccumData: in the bus block's accumulator region (in place: the serial post-process
// and contexts that leave the post-process to their caller work there) or where the fused post-process filed it.
const float *CarrySource(oalgpu_context *c, bool carry)
{
    const float *src = nullptr;
    if(carry && c->L.hrtf) src = c->carryInBuf ? c->carryBuf.p : c->L.bus + BusAccumOffset(c->L);
    c->carryInBuf = false;                  // the reduction's result -- partial sums + carry -- is in the bus block again
    return src;
}

// BandSplitter::processHfScale's state transition over a run of `seg` samples of silence (core/filters/splitter.cpp:65-97: the
// recurrence SplitStep<true> of dev_wave.hpp, same operations): lower triangular in (lp_z1, lp_z2), decoupled in ap_z1 --
// [[p, 0, 0], [q, r, 0], [0, 0, s]].  Data independent and the same for every channel: raised here, once per update size, instead
// of by every wavefront that scans a channel.
static void SplitterRunPowers(float coeff, uint32_t seg, float out[4])
{
    const float ap = coeff, lp = coeff * 0.5f + 0.5f;
    float st[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
    for(uint32_t i = 0; i < seg; ++i)
        for(auto &v : st)
        {
            const float d0 = (0.0f - v[0]) * lp;
            const float lpY0 = v[0] + d0;
            v[0] = std::fmaf(d0, lp, lpY0);
            const float d1 = (lpY0 - v[1]) * lp;
            const float lpY1 = v[1] + d1;
            v[1] = lpY1 + d1;
            const float apY = std::fmaf(0.0f, ap, v[2]);
            v[2] = std::fmaf(-apY, ap, 0.0f);
        }
    out[0] = st[0][0]; out[1] = st[0][1]; out[2] = st[1][1]; out[3] = st[2][2];
}

// MixDirectHrtf of a FAST wavefront-kernel context in one launch (post_wave.hip): reads the bus block's accumulator, leaves the
// shifted accumulator in carryBuf and the new splitter states in the other state buffer.
// resident: the update's reduction is BusReduceResidentKernel on the reduce stream (ResidentSubmit): the launch waits for ITS
// counter and counts itself in for the next one.
// The counters the kernels wait for only ever grow and the host keeps what they will read (postEpoch, reducedEpoch, outSeq, the
// resident targets): those mirrors move only once the launch has been accepted -- a failed launch must not leave every later
// one waiting for a count that never comes.
int PostDirectHrtfFused(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do, hipEvent_t evDone, bool resident)
{
    const DeviceLayout &L = c->L;
    float *left = L.bus + size_t{L.numDry} * kLine;
    SplitterState *spIn = c->dSplitCur ? c->dSplit2.p : c->dSplit.p, *spOut = c->dSplitCur ? c->dSplit.p : c->dSplit2.p;
    const uint32_t postEpoch = c->postEpoch + L.numDry;    // what the channel counter reads when this update's channels have all arrived
    const uint32_t seg = ((samples_to_do + 63u) / 64u) | 1u;
    if(c->runPowerSeg != seg) { SplitterRunPowers(c->dSplitCoeff, seg, c->runPower); c->runPowerSeg = seg; }
    const uint32_t slot = c->outNext % oalgpu_context::kIoSlots;
    const bool ring = c->outRing && c->outFlags;
    const uint32_t outTarget = c->outArrivedTotal + PostResidentFirGroups();
    const PostHrtfCall call{left, left + kLine, L.bus, L.numDry, L.bus + BusAccumOffset(L), c->carryBuf.p, spIn, spOut, c->dHfScale.p, c->dCoeffs.p,
        c->dIrSize, samples_to_do, c->dTemp.p, c->postArrived.p, postEpoch, c->runPower, evDone, ring ? c->outHost[slot] : nullptr,
        ring ? c->outFlags + size_t{slot} * 16 : nullptr, c->outSeq + 1u};
    auto &R = c->res;
    if(resident)
    {
        c->reduceHeld = false;
        LaunchPostResident(s, call, R.counters.p, R.hostFlags, (R.posts + 1u) * R.redGroups, (R.posts + 1u) * R.firGroups, R.posts + 1u);
        HIP_TRY(hipGetLastError());
        ++R.posts;
    }
    else if(c->reduceHeld)
    {   // the update's reduction rides in the same launch (its partial buses: heldL's)
        c->reduceHeld = false;
        if(!c->reducedCount.p) { HIP_TRY(c->reducedCount.alloc(1)); HIP_TRY(c->reducedCount.zero()); }
        const uint32_t reducedEpoch = c->reducedEpoch + ReducePostReduceGroups(c->heldL);
        LaunchReducePostFused(s, call, c->heldL, CarrySource(c, c->carryAccum && L.hrtf), c->outArrived.p, outTarget, c->reducedCount.p, reducedEpoch);
        HIP_TRY(hipGetLastError());
        c->reducedEpoch = reducedEpoch;
        if(ring) c->outArrivedTotal = outTarget;
    }
    else
    {
        LaunchPostDirectHrtfFused(s, call, c->outArrived.p, outTarget);
        HIP_TRY(hipGetLastError());
        if(ring) c->outArrivedTotal = outTarget;
    }
    c->postEpoch = postEpoch;
    if(ring) c->outSlotSeq[slot] = ++c->outSeq;
    c->outRingWritten = ring;
    c->dSplitCur ^= 1u;
    c->carryInBuf = true;
    return OALGPU_OK;
}

// The held reduction of an update whose dry lines have no writer (RunMixUpdate: silentPost), with what is left of its post-process
// in the same launch (BusReduceShiftKernel, voice_kernel.hip).  The carried accumulator alternates between carryBuf and the bus
// block's accumulator region: the launch reads one and files the shifted one in the other, and carryInBuf says where it is --
// to the next reduction of either path (CarrySource) and to oalgpu_read_hrtf_accum.  No PostFusedKernel runs: its channel counter
// (postEpoch) and the splitter states (dSplitCur) stay where they are.
static int ReduceShiftSilent(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do, hipEvent_t evDone)
{
    c->reduceHeld = false;
    float *left = c->L.bus + size_t{c->L.numDry} * kLine;
    const uint32_t slot = c->outNext % oalgpu_context::kIoSlots;
    const bool ring = c->outRing && c->outFlags;
    const uint32_t outTarget = c->outArrivedTotal + BusReduceShiftGroups();
    const bool wasInBuf = c->carryInBuf;
    const float *carry = CarrySource(c, c->carryAccum);
    float *carryOut = wasInBuf ? c->L.bus + BusAccumOffset(c->L) : c->carryBuf.p;
    LaunchBusReduceShift(s, c->heldL, carry, carryOut, left, left + kLine, samples_to_do, evDone, ring ? c->outHost[slot] : nullptr,
        ring ? c->outFlags + size_t{slot} * 16 : nullptr, c->outSeq + 1u, c->outArrived.p, outTarget);
    HIP_TRY(hipGetLastError());
    if(ring) { c->outArrivedTotal = outTarget; c->outSlotSeq[slot] = ++c->outSeq; }
    c->outRingWritten = ring;
    c->carryInBuf = !wasInBuf;
    ++c->silentPosts;
    return OALGPU_OK;
}

// Orders the main stream behind whatever a pipelined oalgpu_mix_update left on the post stream.
int JoinPost(oalgpu_context *c)
{
    if(!c->postPending) return OALGPU_OK;
    HIP_TRY(hipStreamWaitEvent(c->stream, c->lastPostEvent ? c->lastPostEvent : c->evPostDone, 0));
    c->postPending = false;
    return OALGPU_OK;
}

// ---- the update's entry points ----
static int RefuseWithoutHrtfData(const oalgpu_context *c)
{
    if(c->L.hrtf && !c->hrtfLoaded) return Fail(OALGPU_ERR_NO_HRTF, "HRTF context without a data set");
    return OALGPU_OK;
}

// What every update entry point starts with, like BeginSetter for the setters.  The refusals, in this order: a null context or a
// sample count outside a line; (kNeedsFast) a context that does not pipeline two streams of its own; an attached context, which
// its device context updates; (kNeedsHrtfData) an HRTF context without a data set.
enum : uint32_t { kNeedsFast = 1u, kNeedsHrtfData = 2u };
static int BeginUpdate(oalgpu_context *c, const char *who, uint32_t samples_to_do, uint32_t needs = 0u)
{
    if(!c || samples_to_do == 0 || samples_to_do > kLine) return Fail(OALGPU_ERR_INVALID, "samples_to_do must be 1..1024");
    if((needs & kNeedsFast) && !(c->useWave && c->ownStream))
        return Fail(OALGPU_ERR_INVALID, std::string(who) + ": needs a FAST context (wavefront kernel) on its own streams");
    if(int rc = RefuseAttached(c, who)) return rc;
    return (needs & kNeedsHrtfData) ? RefuseWithoutHrtfData(c) : OALGPU_OK;
}

// in front of a context's voice kernel: its callback sources are asked, its attached contexts' voices go first
static int BeforeVoices(oalgpu_context *c, uint32_t samples_to_do)
{
    if(!c->cbVoices.empty()) { if(int rc = ServiceCallbacks(c, samples_to_do)) return rc; }
    if(!c->attached.empty()) { if(int rc = MixAttached(c, samples_to_do)) return rc; }
    c->outRingWritten = false;
    return OALGPU_OK;
}

// the end of a timed update (oalgpu_set_timing) on stream `s`
static int EndTimedUpdate(oalgpu_context *c, hipStream_t s)
{
    if(!c->timing) return OALGPU_OK;
    HIP_TRY(hipEventRecord(c->evEnd, s));
    c->timed = true;
    return OALGPU_OK;
}

int oalgpu_mix_voices(oalgpu_context *c, uint32_t samples_to_do)
{
    if(int rc = BeginUpdate(c, "oalgpu_mix_voices", samples_to_do)) return rc;
    return MixVoicesSerial(c, samples_to_do);
}

// oalgpu_mix_voices; also what a device context does for each of its attached contexts (which pass no entry point: the data set
// is asked for here)
int MixVoicesSerial(oalgpu_context *c, uint32_t samples_to_do)
{
    if(int rc = RefuseWithoutHrtfData(c)) return rc;
    if(int rc = UseCtx(c)) return rc;
    if(int rc = FlushInits(c)) return rc;
    if(int rc = JoinPost(c)) return rc;
    if(int rc = BeforeVoices(c, samples_to_do)) return rc;
    if(c->useWave)    // (timing: the two events are bound to the dispatch itself -- the kernel's own start and end)
        HIP_TRY(LaunchVoiceWave(c->stream, c->L, samples_to_do, c->profArg(), c->timing ? c->evStart : nullptr, c->timing ? c->evVoice : nullptr));
    else
    {
        if(c->timing) HIP_TRY(hipEventRecord(c->evStart, c->stream));
        HIP_TRY(LaunchVoiceMix(c->stream, c->exact, c->L, samples_to_do, c->carryAccum));
        if(c->timing) HIP_TRY(hipEventRecord(c->evVoice, c->stream));
    }
    // (an attached context's bus block is single-buffered: the device context's merge of the update before reads it)
    if(c->attachedTo && c->attachedTo->mergeInFlight) HIP_TRY(hipStreamWaitEvent(c->stream, c->attachedTo->evMerged, 0));
    // the wavefront kernel leaves the carried HRTF accumulator tail to the reduction
    LaunchBusReduce(c->stream, c->L, samples_to_do, CarrySource(c, c->useWave && c->carryAccum));
    HIP_TRY(hipGetLastError());
    if(int rc = CommReduceBus(c, c->stream)) return rc;
    return EndTimedUpdate(c, c->stream);
}

int oalgpu_post_process(oalgpu_context *c, uint32_t samples_to_do)
{
    if(int rc = BeginUpdate(c, "oalgpu_post_process", samples_to_do)) return rc;
    if(int rc = UseCtx(c)) return rc;
    if(int rc = JoinPost(c)) return rc;
    if(!c->attached.empty()) { if(int rc = MergeAttached(c, c->stream, samples_to_do)) return rc; }
    if(int rc = RunEffects(c, c->stream, samples_to_do)) return rc;
    if(!c->L.hrtf)
    {
        if(int rc = RunSpeakerPost(c, c->stream, samples_to_do)) return rc;
        return EndTimedUpdate(c, c->stream);
    }
    const DeviceLayout &L = c->L;
    if(L.numReal < 2) return Fail(OALGPU_ERR_INVALID, "HRTF post-process needs two real output lines");
    float *left = L.bus + size_t{L.numDry} * kLine;
    float *right = left + kLine;
    // (the wavefront-kernel contexts carry the accumulator through their reduction: the one-launch form; the others mix it in place)
    SplitterState *spCur = c->dSplitCur ? c->dSplit2.p : c->dSplit.p;
    if(c->exact)
        LaunchMixDirectHrtf(c->stream, true, left, right, L.bus, L.numDry, L.bus + BusAccumOffset(L), spCur,
            c->dHfScale.p, c->dCoeffs.p, c->dIrSize, samples_to_do, c->dTemp.p);
    else if(c->useWave) { if(int rc = PostDirectHrtfFused(c, c->stream, samples_to_do, nullptr)) return rc; }
    else
        LaunchPostDirectHrtfFast(c->stream, left, right, L.bus, L.numDry, L.bus + BusAccumOffset(L), spCur,
            c->dHfScale.p, c->dCoeffs.p, c->dIrSize, samples_to_do, c->dTemp.p);
    HIP_TRY(hipGetLastError());
    if(int rc = RunLimiter(c, c->stream, samples_to_do)) return rc;
    return EndTimedUpdate(c, c->stream);
}

static int RunMixUpdate(oalgpu_context *c, uint32_t samples_to_do, int post_process, oalgpu_param_block *next);
static void PlanPost(oalgpu_context *c, int post_process);
static int GuardPartialSet(oalgpu_context *c, uint32_t p);
static int GuardPartialSets(oalgpu_context *c, const uint32_t *sets, uint32_t count);
static int ReduceBehindVoices(oalgpu_context *c, const DeviceLayout &L, uint32_t p, uint32_t samples_to_do);

// How many deferred updates ONE voice launch of the context may cover right now (1: a launch per update).  A launch spans updates
// only where nothing has to happen on the host or on another context between two of them: no callback sources, no attached
// contexts, no collective, no deferred starts, no measurement variant.
static uint32_t SpanLimit(const oalgpu_context *c)
{
    if(c->launchSpan == 1u || c->numSets < oalgpu_context::kPartSets || !Wave16HasSpan(c->L)) return 1u;
    if(!c->cbVoices.empty() || !c->attached.empty() || c->attachedTo || c->comm || c->timing || !c->initPending.empty() || c->prof.times) return 1u;
    return c->launchSpan ? c->launchSpan : kSpanMax;
}

int oalgpu_mix_update(oalgpu_context *c, uint32_t samples_to_do, int post_process)
{
    if(int rc = BeginUpdate(c, "oalgpu_mix_update", samples_to_do, kNeedsHrtfData)) return rc;
    if(c->res.cooldown) --c->res.cooldown;
    else if(ResidentWanted(c, post_process))
    {   // the resident voice kernel: a doorbell, the update's reduction and its post-process
        const int rc = ResidentSubmit(c, samples_to_do);
        if(rc <= 0) return rc;                       // (1: the mode is not available after all -- on to the launched path)
    }
    const bool defers = c->useWave && c->ownStream && !c->serialOnly && !c->timing && (c->desc.flags & OALGPU_CTX_APPLY_IN_VOICE_KERNEL)
        && WaveKernelAppliesRecords(c->L) && !(c->res.enabled && !c->res.failed && !c->res.cooldown);
    // deferred updates whose blocks have all been handed over, and room in the launch that will cover them: this one joins them
    auto &Q = c->pendingMix;
    if(defers && Q.count && Q.count < SpanLimit(c) && Q.u[Q.count - 1u].behind && !c->res.pendingBlock)
    {
        if(int rc = UseDevice(c->desc.device)) return rc;
        Q.u[Q.count++] = oalgpu_context::PendingUpdate{samples_to_do, post_process, nullptr};
        return OALGPU_OK;
    }
    if(int rc = UseCtx(c)) return rc;                // (submits the updates deferred before this one)
    if(defers)
    {   // submitted with a later library call on this context (see pendingMix); whatever goes wrong then is that call's error
        Q.u[0] = oalgpu_context::PendingUpdate{samples_to_do, post_process, nullptr};
        Q.count = 1;
        return OALGPU_OK;
    }
    return RunMixUpdate(c, samples_to_do, post_process, nullptr);
}

int oalgpu_context_set_launch_span(oalgpu_context *c, uint32_t n)
{
    if(int rc = BeginSetter(c, "oalgpu_context_set_launch_span")) return rc;
    if(n > kSpanMax) return Fail(OALGPU_ERR_INVALID, "oalgpu_context_set_launch_span: 0 (automatic), 1 (never) or 2 .. 4 updates per launch");
    c->launchSpan = n;
    return OALGPU_OK;
}

int oalgpu_context_launch_stats(oalgpu_context *c, uint64_t spans[4], uint64_t *silent_posts)
{
    if(!c) return Fail(OALGPU_ERR_INVALID, "null argument");
    static_assert(kSpanMax == 4, "oalgpu.h says four");
    if(spans) for(uint32_t i = 0; i < kSpanMax; ++i) spans[i] = c->spanCounts[i];
    if(silent_posts) *silent_posts = c->silentPosts;
    return OALGPU_OK;
}

int oalgpu_context_guard_stats(oalgpu_context *c, uint64_t *main_stream_guards, uint64_t *guard_queries)
{
    if(!c) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(main_stream_guards) *main_stream_guards = c->mainStreamGuards;
    if(guard_queries) *guard_queries = c->guardQueries;
    return OALGPU_OK;
}

// oalgpu_param_block_apply on a context whose newest deferred update has no block behind it yet: the block goes there, and the
// queue is submitted if the launch that covers it is full -- or, under the automatic rule, if the main stream has nothing to do
// (the last voice launch has ended: holding updates back would leave the GPU idle).  A host that waits for every update's output
// thus gets a launch per update; one that runs ahead of the GPU gets launches that span its lead.
int DeferBlockBehindPending(oalgpu_context *c, oalgpu_param_block *b)
{
    auto &Q = c->pendingMix;
    Q.u[Q.count - 1u].behind = b;
    b->queuedBy = c;
    bool submit = Q.count >= SpanLimit(c);
    if(!submit && c->launchSpan == 0u)
        submit = !c->lastVoiceEvent || hipEventQuery(c->lastVoiceEvent) != hipErrorNotReady;
    return submit ? FlushPendingMix(c) : OALGPU_OK;
}

int BeginSetter(oalgpu_context *c, const char *who)
{
    if(!c) return Fail(OALGPU_ERR_INVALID, std::string(who) + ": null context");
    if(int rc = FlushPendingMix(c)) return rc;
    return c->res.pendingBlock ? UseCtx(c) : OALGPU_OK;
}

static int RunMixSpan(oalgpu_context *c, const oalgpu_context::PendingUpdate *u, uint32_t count);

int FlushPendingMix(oalgpu_context *c)
{
    // (a setter of an attached context: the device context's deferred update mixes this context's voices as they were)
    if(c->attachedTo) { if(int rc = FlushPendingMix(c->attachedTo)) return rc; }
    if(!c->pendingMix.active()) return OALGPU_OK;
    const auto Q = c->pendingMix;
    c->pendingMix.count = 0;
    for(uint32_t i = 0; i < Q.count; ++i) if(Q.u[i].behind) Q.u[i].behind->queuedBy = nullptr;
    if(Q.count > 1u && Q.count <= SpanLimit(c)) return RunMixSpan(c, Q.u, Q.count);
    for(uint32_t i = 0; i < Q.count; ++i) { if(int rc = RunMixUpdate(c, Q.u[i].samples, Q.u[i].post, Q.u[i].behind)) return rc; }
    return OALGPU_OK;
}

// next: a parameter block the update's voice kernel installs behind the voices it mixed (null: none)
static int RunMixUpdate(oalgpu_context *c, uint32_t samples_to_do, int post_process, oalgpu_param_block *next)
{
    c->nextRecs = next ? next->recs.p : nullptr;
    c->nextMap = next ? next->voiceToRec.p : nullptr;
    c->nextRows = next ? next->rows.p : nullptr;
    struct Clear { oalgpu_context *c; ~Clear() { c->nextRecs = nullptr; c->nextMap = nullptr; c->nextRows = nullptr; } } clear{c};
    if(!(c->useWave && c->ownStream) || c->serialOnly)
    {   // one stream: the workgroup-per-voice-group kernel reads the carried accumulator itself,
        // and a caller-owned stream (RCCL ordering) is never forked
        if(int rc = oalgpu_mix_voices(c, samples_to_do)) return rc;
        if(post_process && c->commRank == 0) return oalgpu_post_process(c, samples_to_do);
        return OALGPU_OK;
    }
    PlanPost(c, post_process);
    struct ClearSilent { oalgpu_context *c; ~ClearSilent() { c->silentPost = false; } } clearSilent{c};
    const int rcv = oalgpu_mix_voices_overlapped(c, samples_to_do);
    c->fuseReduce = false;
    if(rcv) { c->reduceHeld = false; return rcv; }
    // sharded contexts: the effects and the post-process run where the reduced buses are, on rank 0
    return oalgpu_post_process_overlapped(c, samples_to_do, post_process && c->commRank == 0);
}

// how a pipelined update's reduction and post-process are launched: fuseReduce, silentPost
static void PlanPost(oalgpu_context *c, int post_process)
{
    const bool oneLaunch = post_process && !c->comm && c->L.hrtf && c->L.numSlots == 0 && c->L.numReal >= 2 && !c->timing && c->attached.empty();
    // Nothing writes the dry lines of such a context (the voices mix into the accumulator, the reduction zero-fills the lines), so its
    // post-process adds nothing: the reduction forms the output lines and shifts the accumulator itself (ReduceShiftSilent).  Sticky:
    // once something else may have written the lines -- an attached context, a collective, a caller that holds the bus pointer --
    // the splitters may hold state, and the context keeps the whole chain.
    // Only where updates are deferred (OALGPU_CTX_APPLY_IN_VOICE_KERNEL): with a parameter kernel between two voice kernels the
    // short post chain measured 1 us per step SLOWER than the whole one (35.7 -> 36.7 us, profiles/launch_span/fourway_xflags.txt),
    // and it pays only together with a voice launch that spans updates.
    if(!c->attached.empty() || c->comm) c->dryWriter = true;
    c->silentPost = oneLaunch && !c->dryWriter && !c->limOn && (c->desc.flags & OALGPU_CTX_APPLY_IN_VOICE_KERNEL) && !(c->desc.flags & OALGPU_CTX_FULL_POST);
    c->fuseReduce = c->silentPost || (oneLaunch && (c->desc.flags & OALGPU_CTX_FUSED_REDUCE));
}

// ONE voice launch over `count` deferred updates (the bounded run of voice_wave16.hip), then on the post stream what each of
// them has there after a launch of its own, in order: its reduction and its post-process, with its own partial set, events,
// output lines and ring slot.  What oalgpu_mix_voices_overlapped does in front of a launch is done for every update it covers.
static int RunMixSpan(oalgpu_context *c, const oalgpu_context::PendingUpdate *u, uint32_t count)
{
    if(int rc = UseDevice(c->desc.device)) return rc;
    if(int rc = FlushResidentBlock(c)) return rc;
    c->outRingWritten = false;
    SpanUpdates span{};
    span.count = count;
    uint32_t sets[kSpanMax];
    for(uint32_t i = 0; i < count; ++i) sets[i] = (c->parity + i) % c->numSets;
    if(int rc = GuardPartialSets(c, sets, count)) return rc;
    for(uint32_t i = 0; i < count; ++i)
    {
        const uint32_t p = sets[i];
        const oalgpu_param_block *b = u[i].behind;
        span.samples[i] = u[i].samples;
        span.recs[i] = b ? b->recs.p : nullptr; span.map[i] = b ? b->voiceToRec.p : nullptr; span.rows[i] = b ? b->rows.p : nullptr;
        span.part[i] = c->partHrtfBuf[p];
    }
    hipEvent_t evVoice = c->evVoiceDone[c->voiceLaunches++ & 1u];
    HIP_TRY(LaunchVoiceWave16Span(c->stream, c->L, span, evVoice));
    ++c->spanCounts[count - 1u];
    c->lastVoiceEvent = evVoice;
    c->parity = (c->parity + count) % c->numSets;
    HIP_TRY(hipStreamWaitEvent(c->postStream, evVoice, 0));
    for(uint32_t i = 0; i < count; ++i)
    {
        DeviceLayout L = c->L;
        L.partHrtf = span.part[i];
        PlanPost(c, u[i].post);
        struct ClearSilent { oalgpu_context *c; ~ClearSilent() { c->silentPost = false; c->fuseReduce = false; } } clearSilent{c};
        if(int rc = ReduceBehindVoices(c, L, sets[i], u[i].samples)) { c->reduceHeld = false; return rc; }
        if(int rc = oalgpu_post_process_overlapped(c, u[i].samples, u[i].post && c->commRank == 0)) return rc;
    }
    return OALGPU_OK;
}

// in front of a voice launch that writes partial set p: the set was last read by the reduction of numSets updates ago
// (almost always long done: then no barrier packet goes into the main queue in front of the voice kernel)
static int GuardPartialSet(oalgpu_context *c, uint32_t p) { return GuardPartialSets(c, &p, 1u); }

// The same in front of a voice launch that writes `count` sets, in the order of its updates: ONE query and at most ONE wait.  The
// reductions run in order on one stream (the post stream; with the whole post chain between them as well), so the event of the
// newest one that read any of the sets stands for them all -- four waits were four barrier packets in the main queue, each
// taken up only when the launch before had ended (5 us apiece between two launches, profiles/span_guard).  An event found ready
// proves every update up to its own reduced: launches to come skip the query.
static int GuardPartialSets(oalgpu_context *c, const uint32_t *sets, uint32_t count)
{
    uint32_t newest = sets[0];
    for(uint32_t i = 1; i < count; ++i) if(c->reduceUpdate[sets[i]] > c->reduceUpdate[newest]) newest = sets[i];
    if(c->reduceUpdate[newest] > c->updatesKnownDone)
    {
        hipEvent_t ev = c->evReduceDone[newest];
        const hipError_t q = hipEventQuery(ev);
        ++c->guardQueries;
        if(q == hipErrorNotReady) { HIP_TRY(hipStreamWaitEvent(c->stream, ev, 0)); ++c->mainStreamGuards; }
        else { HIP_TRY(q); c->updatesKnownDone = c->reduceUpdate[newest]; }
    }
    for(uint32_t i = 0; i < count; ++i) c->reduceUpdate[sets[i]] = ++c->updatesSubmitted;
    return OALGPU_OK;
}

// post stream, behind the wait for the voice launch: the reduction of the update whose partial buses are L's (set p) -- or, held
// back, its hand-over to the post-process that follows at once and launches it with itself (fuseReduce)
static int ReduceBehindVoices(oalgpu_context *c, const DeviceLayout &L, uint32_t p, uint32_t samples_to_do)
{
    if(c->fuseReduce)
    {
        c->reduceHeld = true; c->heldL = L; c->heldParity = p;
        return OALGPU_OK;
    }
    LaunchBusReduce(c->postStream, L, samples_to_do, CarrySource(c, c->carryAccum && L.hrtf), true, c->evReduceDone[p]);
    HIP_TRY(hipGetLastError());
    return CommReduceBus(c, c->postStream);                      // beside the next update's voice kernel
}

/* `count` consecutive updates in one call: update i applies param_blocks[i] (the array or an entry may be NULL) and mixes
 * -- the loop a C++ host would write, without a language binding's per-call cost between the submissions */
int oalgpu_mix_update_run(oalgpu_context *c, oalgpu_param_block *const *param_blocks, uint32_t count, uint32_t samples_to_do,
    int post_process)
{
    if(!c || count == 0) return Fail(OALGPU_ERR_INVALID, "oalgpu_mix_update_run: bad arguments");
    if(int rc = RefuseAttached(c, "oalgpu_mix_update_run")) return rc;
    for(uint32_t i = 0; i < count; ++i)
    {
        if(param_blocks && param_blocks[i]) { if(int rc = oalgpu_param_block_apply(c, param_blocks[i])) return rc; }
        if(int rc = oalgpu_mix_update(c, samples_to_do, post_process)) return rc;
    }
    return OALGPU_OK;
}

int oalgpu_mix_voices_overlapped(oalgpu_context *c, uint32_t samples_to_do)
{
    if(int rc = BeginUpdate(c, "oalgpu_mix_voices_overlapped", samples_to_do, kNeedsFast | kNeedsHrtfData)) return rc;
    if(int rc = UseCtx(c)) return rc;
    if(int rc = FlushInits(c)) return rc;
    if(int rc = BeforeVoices(c, samples_to_do)) return rc;
    const uint32_t p = c->parity;
    DeviceLayout L = c->L;
    L.partHrtf = c->partHrtfBuf[p];
    if(L.streams || L.accLines || L.rows8) L.partLines = c->partLinesBuf[p];
    // main stream: this update's voices
    if(int rc = GuardPartialSet(c, p)) return rc;
    hipEvent_t evVoice = c->evVoiceDone[c->voiceLaunches++ & 1u];
    // (timing: the two events are bound to the dispatch itself -- the kernel's own start and end)
    // The event the post stream waits for is bound to the voice kernel's dispatch (hipExtLaunchKernel's stop event: one
    // runtime call less per update than a record behind the launch).  Timing runs use that slot for their own event.
    HIP_TRY(LaunchVoiceWave(c->stream, L, samples_to_do, c->profArg(), c->timing ? c->evStart : nullptr, c->timing ? c->evVoice : evVoice,
        c->nextRecs, c->nextMap, c->nextRows));
    if(c->timing) HIP_TRY(hipEventRecord(evVoice, c->stream));
    ++c->spanCounts[0];
    c->lastVoiceEvent = evVoice;
    // post stream: the reduction (adds the carried HRTF accumulator tail); whatever follows on that stream -- a collective, the effects, the post-process -- runs beside
    // the next update's parameter and voice kernels
    HIP_TRY(hipStreamWaitEvent(c->postStream, evVoice, 0));
    // (4-wavefront workgroups: they find room on a CU as soon as ONE of the next update's voice workgroups
    // has left it; the 16-wavefront form waits for a whole CU -- measured 62 against 53 us per config-2 step)
    c->parity = (p + 1u) % c->numSets;
    return ReduceBehindVoices(c, L, p, samples_to_do);
}

void *oalgpu_post_stream(oalgpu_context *c) { return c ? static_cast<void*>(c->postStream) : nullptr; }

int oalgpu_post_process_overlapped(oalgpu_context *c, uint32_t samples_to_do, int post_process)
{
    if(int rc = BeginUpdate(c, "oalgpu_post_process_overlapped", samples_to_do, kNeedsFast)) return rc;
    if(post_process && c->L.hrtf && c->L.numReal < 2) return Fail(OALGPU_ERR_INVALID, "HRTF post-process needs two real output lines");
    if(int rc = UseCtx(c)) return rc;
    const DeviceLayout &L = c->L;
    bool postDoneBound = false;
    if(post_process && !c->attached.empty()) { if(int rc = MergeAttached(c, c->postStream, samples_to_do)) return rc; }
    if(post_process) { if(int rc = RunEffects(c, c->postStream, samples_to_do)) return rc; }
    if(post_process && L.hrtf)
    {
        // (the update's last launch on this stream, unless timing asks for an event of its own behind it: evPostDone rides on it)
        // (with the reduction in the same launch the event is the one the voice kernel of two updates on waits for as well)
        // (a limiter is the update's last launch instead: evPostDone is recorded behind it)
        hipEvent_t ev = c->reduceHeld ? c->evReduceDone[c->heldParity] : ((c->timing || c->limOn) ? nullptr : c->evPostDone);
        c->lastPostEvent = (ev && !c->limOn) ? ev : c->evPostDone;
        if(c->reduceHeld && c->silentPost) { if(int rc = ReduceShiftSilent(c, c->postStream, samples_to_do, ev)) return rc; }
        else if(int rc = PostDirectHrtfFused(c, c->postStream, samples_to_do, ev)) return rc;
        postDoneBound = ev != nullptr && !c->limOn;
        if(int rc = RunLimiter(c, c->postStream, samples_to_do)) return rc;
    }
    else
    {
        c->lastPostEvent = c->evPostDone;
        if(post_process) { if(int rc = RunSpeakerPost(c, c->postStream, samples_to_do)) return rc; }
    }
    if(int rc = EndTimedUpdate(c, c->postStream)) return rc;
    if(!postDoneBound) HIP_TRY(hipEventRecord(c->evPostDone, c->postStream));
    c->postPending = true;
    return OALGPU_OK;
}

int oalgpu_sync(oalgpu_context *c)
{
    if(!c) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(int rc = UseCtx(c)) return rc;           // (a resident voice kernel finishes what has been rung and ends)
    HIP_TRY(hipStreamSynchronize(c->stream));
    if(c->res.reduceStream) HIP_TRY(hipStreamSynchronize(c->res.reduceStream));
    if(c->postStream) HIP_TRY(hipStreamSynchronize(c->postStream));
    c->postPending = false;
    c->updatesKnownDone = c->updatesSubmitted;
    for(oalgpu_context *a : c->attached)
    {   // (their work of the update: the voices and reductions of an update that merged nothing are waited for too)
        HIP_TRY(hipStreamSynchronize(a->stream));
        if(a->postStream) HIP_TRY(hipStreamSynchronize(a->postStream));
        a->postPending = false;
        a->updatesKnownDone = a->updatesSubmitted;
    }
    c->mergeInFlight = false;
    if(c->res.ready) { ResidentCollectTimes(c, true); if(int rc = ResidentCheckError(c)) return rc; }
    return OALGPU_OK;
}

int oalgpu_set_timing(oalgpu_context *c, int enable)
{
    if(int rc = BeginSetter(c, "oalgpu_set_timing")) return rc;
    c->timing = enable != 0;
    c->timed = false;
    return OALGPU_OK;
}

int oalgpu_last_update_ms(oalgpu_context *c, float *total_ms, float *voice_kernel_ms)
{
    if(!c || !c->timed) return Fail(OALGPU_ERR_INVALID, "no timed update (call oalgpu_set_timing first)");
    if(int rc = oalgpu_sync(c)) return rc;
    if(total_ms) HIP_TRY(hipEventElapsedTime(total_ms, c->evStart, c->evEnd));
    if(voice_kernel_ms) HIP_TRY(hipEventElapsedTime(voice_kernel_ms, c->evStart, c->evVoice));
    return OALGPU_OK;
}

#ifdef OALGPU_MEASUREMENT      // (liboalgpu_measure.so, `make measure`: tools/measure/oalgpu_measure.h)
/* Measurement aid, OALGPU_CTX_PROFILE contexts: which stages the voice kernel's measurement variant skips
 * (1 FIR, 2 resampler, 8 direct filter, 16 FIR input build); 0 = none. */
int oalgpu_debug_set_ablate(oalgpu_context *c, uint32_t mask)
{
    if(!c || !c->phaseTimes.p) return Fail(OALGPU_ERR_INVALID, "not an OALGPU_CTX_PROFILE context");
    c->prof.ablate = mask;
    return OALGPU_OK;
}

/* Measurement aid: copies the [voice][8] s_memtime stamps the voice kernel's measurement variant
 * recorded (contexts created with OALGPU_CTX_PROFILE). */
int oalgpu_debug_phase_times(oalgpu_context *c, unsigned long long *out)
{
    if(!c || !out || !c->phaseTimes.p) return Fail(OALGPU_ERR_INVALID, "phase times were not enabled");
    if(int rc = oalgpu_sync(c)) return rc;
    HIP_TRY(hipMemcpy(out, c->phaseTimes.p, size_t{c->L.numVoices} * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return OALGPU_OK;
}

/* Same aid: the [wavefront][4] stamps behind them (kernel entry, first voice requested and parked,
 * last voice done, partial bus stored; then pass 0 in detail: first control line in registers, first request issued,
 * workgroup through the table-staging barrier); `out` holds numVoices*8 words ([wavefront][8]), *waves receives the count. */
int oalgpu_debug_wave_times(oalgpu_context *c, unsigned long long *out, uint32_t *waves)
{
    if(!c || !out || !waves || !c->phaseTimes.p) return Fail(OALGPU_ERR_INVALID, "phase times were not enabled");
    if(int rc = oalgpu_sync(c)) return rc;
    HIP_TRY(hipMemcpy(out, c->phaseTimes.p + size_t{c->L.numVoices} * 8, size_t{c->L.numVoices} * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *waves = WaveKernelGroups(c->L) * 4u;
    return OALGPU_OK;
}

#endif // OALGPU_MEASUREMENT

const char *oalgpu_voice_kernel_name(oalgpu_context *c)
{
    if(!c) return "";
    if(c->useWave) return WaveKernelName(c->L);
    return c->exact ? "VoiceMixKernel<true, LINES>" : "VoiceMixKernel<false, LINES>";
}

/* Multi-GPU: whether this context's voice kernel continues the carried HRTF accumulator tail
 * (exactly one rank must, the one that runs the post-process on the reduced buses). */
int oalgpu_set_carry_accum(oalgpu_context *c, int enable)
{
    if(int rc = BeginSetter(c, "oalgpu_set_carry_accum")) return rc;
    c->carryAccum = enable != 0;
    return OALGPU_OK;
}
