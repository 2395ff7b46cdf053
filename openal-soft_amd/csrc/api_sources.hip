// 3D source parameters computed on the GPU: the listener, the slots' send environments, and the entry points that turn source
// properties into parameter records with SourceParamsKernel (source_kernels.hip) -- and the same arithmetic (dev_source.hpp)
// compiled for the host, oalgpu_source_params_host.
#include "api_context.hpp"

namespace {

// the resampler tables' constants as the stage reads them (BSincTable without the filters; where the blob keeps the filters)
const ResamplerConsts &HostResamplerConsts()
{
    static const ResamplerConsts k = [] {
        ResamplerConsts r{};
        const TableBlob &blob = Blob();
        const int fam[3] = {12, 24, 48};
        for(int f = 0; f < 3; ++f)
        {
            const BsincTable *t = GetBsincTable(fam[f]);
            r.fam[f].scaleBase = t->scaleBase; r.fam[f].scaleRange = t->scaleRange;
            std::memcpy(r.fam[f].m, t->m, sizeof(t->m));
            std::memcpy(r.fam[f].filterOffset, t->filterOffset, sizeof(t->filterOffset));
            r.bsincBase[f] = blob.bsincBase[f];
        }
        r.cubicBase[0] = blob.cubicBase[0]; r.cubicBase[1] = blob.cubicBase[1];
        return r;
    }();
    return k;
}

bool PropsOk(const oalgpu_source_props &p, uint32_t numSends, uint32_t numSlots)
{
    if(p.resampler < 0 || p.resampler > OALGPU_RESAMPLER_BSINC48) return false;
    if(p.distance_model < OALGPU_DISTANCE_DISABLE || p.distance_model > OALGPU_DISTANCE_EXPONENT_CLAMPED) return false;
    for(uint32_t s = 0; s < numSends; ++s)
        if(p.send[s].slot >= int32_t(numSlots)) return false;
    return true;
}

// the device side of the stage, allocated with its first use
int EnsureSourceStage(oalgpu_context *c)
{
    if(!c->rsConsts.p)
    {
        HIP_TRY(c->rsConsts.alloc(1));
        HIP_TRY(c->rsConsts.upload(&HostResamplerConsts(), 1));
    }
    if(!c->slotEnv.p)
    {
        c->slotEnvHost.assign(c->L.numSlots, oalgpu_slot_environment{0, 0.0f, 0.0f, 1.0f});
        HIP_TRY(c->slotEnv.alloc(c->L.numSlots));
        if(c->L.numSlots) HIP_TRY(c->slotEnv.upload(c->slotEnvHost.data(), c->L.numSlots));
    }
    return OALGPU_OK;
}

SourceSetup SetupOf(const oalgpu_context *c)
{
    return SourceSetup{c->desc.sample_rate, c->L.numSends, c->L.numSlots, c->L.numDry, c->L.wetChannels, c->L.hrtf,
        c->slotEnv.p, c->rsConsts.p, c->dryMap.p, c->wetMaps.p};
}

// what both entry points refuse, and the source records of what they accept (c->srcHost)
int CollectSources(oalgpu_context *c, const char *who, const uint32_t *voices, const oalgpu_source_props *props, size_t count)
{
    const std::string name(who);
    if(c->L.hrtf && !c->hrtfLoaded) return Fail(OALGPU_ERR_NO_HRTF, name + ": HRTF context without a data set");
    if(c->L.nfc)
        return Fail(OALGPU_ERR_INVALID, name + ": not for contexts with near-field control (the per-voice w0 adjust stays with the host: oalgpu_voice_set_nfc)");
    for(size_t i = 0; i < count; ++i)
    {
        if(voices[i] >= c->L.numVoices) return Fail(OALGPU_ERR_INVALID, name + ": bad voice index");
        if(c->cbOfVoice[voices[i]] >= 0)
            return Fail(OALGPU_ERR_INVALID, name + ": not for callback voices (their step is mirrored on the host: oalgpu_voice_set_params)");
        if(!PropsOk(props[i], c->L.numSends, c->L.numSlots))
            return Fail(OALGPU_ERR_INVALID, name + ": resampler, distance model or send slot out of range");
        if((voices[i] < c->voiceFreq.size() ? c->voiceFreq[voices[i]] : 0u) == 0u)
            return Fail(OALGPU_ERR_INVALID, name + ": the voice has no frequency (start it with oalgpu_voice_init)");
    }
    // of two records of one voice the last wins: the earlier ones do not reach the device (a wavefront per record, in no order)
    std::vector<int32_t> last(c->L.numVoices, -1);
    for(size_t i = 0; i < count; ++i) last[voices[i]] = int32_t(i);
    c->srcHost.clear(); c->srcVoices.clear();
    for(size_t i = 0; i < count; ++i)
    {
        if(last[voices[i]] != int32_t(i)) continue;
        c->srcHost.push_back(SourceRecord{voices[i], c->voiceFreq[voices[i]], props[i]});
        c->srcVoices.push_back(voices[i]);
    }
    return OALGPU_OK;
}

} // namespace

int oalgpu_context_set_listener(oalgpu_context *c, const oalgpu_listener_params *listener)
{
    if(!c || !listener) return Fail(OALGPU_ERR_INVALID, "oalgpu_context_set_listener: null argument");
    if(listener->distance_model < OALGPU_DISTANCE_DISABLE || listener->distance_model > OALGPU_DISTANCE_EXPONENT_CLAMPED)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_context_set_listener: distance model out of range");
    c->listener = *listener;            // (a kernel argument of the launches from now on: nothing in flight reads it)
    return OALGPU_OK;
}

int oalgpu_slot_set_send_environment(oalgpu_context *c, uint32_t slot, int32_t active, float room_rolloff, float decay_time,
    float air_absorption_gain_hf)
{
    if(!c || slot >= c->L.numSlots) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_set_send_environment: bad arguments");
    if(int rc = BeginVoiceCall(c, true, "", true)) return rc;      // (no source launch in flight reads the table)
    if(int rc = EnsureSourceStage(c)) return rc;
    c->slotEnvHost[slot] = oalgpu_slot_environment{active ? 1 : 0, room_rolloff, decay_time, air_absorption_gain_hf};
    HIP_TRY(hipMemcpy(c->slotEnv.p + slot, &c->slotEnvHost[slot], sizeof(oalgpu_slot_environment), hipMemcpyHostToDevice));
    return OALGPU_OK;
}

int oalgpu_voice_set_source_props(oalgpu_context *c, const uint32_t *voices, const oalgpu_source_props *props, size_t count)
{
    if(!c || !voices || !props) return Fail(OALGPU_ERR_INVALID, "oalgpu_voice_set_source_props: null argument");
    if(count == 0) return OALGPU_OK;
    if(int rc = CollectSources(c, "oalgpu_voice_set_source_props", voices, props, count)) return rc;
    if(int rc = BeginVoiceCall(c)) return rc;
    if(int rc = EnsureSourceStage(c)) return rc;
    count = c->srcHost.size();
    if(int rc = StageRecords(c->stream, c->srcDev, c->srcHost.data(), count)) return rc;
    if(c->paramDev.n < count) HIP_TRY(c->paramDev.alloc(count));
    LaunchSourceParams(c->stream, SetupOf(c), c->hrtfDev, c->listener, c->srcDev.p, uint32_t(count), c->paramDev.p);
    HIP_TRY(hipGetLastError());
    LaunchApplyParams(c->stream, c->L, c->paramDev.p, uint32_t(count));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OALGPU_OK;
}

int oalgpu_param_block_create_from_sources(oalgpu_context *c, const uint32_t *voices, const oalgpu_source_props *props, size_t count,
    oalgpu_param_block **out)
{
    if(!c || !voices || !props || !out || count == 0)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_param_block_create_from_sources: bad arguments");
    *out = nullptr;
    if(int rc = CollectSources(c, "oalgpu_param_block_create_from_sources", voices, props, count)) return rc;
    if(int rc = UseCtx(c)) return rc;
    if(int rc = EnsureSourceStage(c)) return rc;
    count = c->srcHost.size();
    voices = c->srcVoices.data();
    auto b = std::make_unique<oalgpu_param_block>();
    b->count = uint32_t(count);
    b->device = c->desc.device;
    b->hrtfGeneration = c->hrtfGeneration;
    HIP_TRY(b->recs.alloc(count));
    if(int rc = StageRecords(c->stream, c->srcDev, c->srcHost.data(), count)) return rc;
    LaunchSourceParams(c->stream, SetupOf(c), c->hrtfDev, c->listener, c->srcDev.p, uint32_t(count), b->recs.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));       // (the staging is free again; the rows below read finished records)
    if(int rc = FinishParamBlock(c, b.get(), voices, count)) return rc;
    *out = b.release();
    return OALGPU_OK;
}

int oalgpu_source_params_host(const oalgpu_context_desc *desc, const oalgpu_listener_params *listener,
    const oalgpu_slot_environment *slots, const uint8_t *dry_index, const float *dry_scale, const uint8_t *wet_index,
    const float *wet_scale, const void *mhr, size_t mhr_size, uint32_t frequency, const oalgpu_source_props *props, size_t count,
    oalgpu_voice_params *out)
{
    if(!desc || !listener || !props || !out || frequency == 0u || desc->sample_rate == 0u)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_source_params_host: bad arguments");
    if(desc->num_aux_sends > OALGPU_MAX_SENDS || desc->num_dry_channels > OALGPU_MAX_OUTPUT_CHANNELS
        || desc->wet_channels > OALGPU_MAX_AMBI_CHANNELS || !dry_index != !dry_scale || !wet_index != !wet_scale)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_source_params_host: bad arguments");
    const uint32_t numDry = desc->num_dry_channels, numSlots = desc->num_slots, wet = desc->wet_channels;
    std::vector<oalgpu_slot_environment> env(numSlots, oalgpu_slot_environment{0, 0.0f, 0.0f, 1.0f});
    if(slots) std::copy(slots, slots + numSlots, env.begin());
    std::vector<AmbiMapEntry> dryMap(numDry), wetMaps(size_t{numSlots} * wet);
    for(uint32_t i = 0; i < numDry; ++i) dryMap[i] = dry_index ? AmbiMapEntry{dry_index[i], dry_scale[i]} : AmbiMapEntry{i, 1.0f};
    for(size_t i = 0; i < wetMaps.size(); ++i)
        wetMaps[i] = wet_index ? AmbiMapEntry{wet_index[i], wet_scale[i]} : AmbiMapEntry{uint32_t(i % wet), 1.0f};
    for(const AmbiMapEntry &m : dryMap) if(m.index >= OALGPU_MAX_AMBI_CHANNELS) return Fail(OALGPU_ERR_INVALID, "ambisonic channel index out of range");
    for(const AmbiMapEntry &m : wetMaps) if(m.index >= OALGPU_MAX_AMBI_CHANNELS) return Fail(OALGPU_ERR_INVALID, "ambisonic channel index out of range");
    HrtfData hrtf;
    HrtfStoreDev store{};
    if(desc->hrtf)
    {
        if(!mhr) return Fail(OALGPU_ERR_NO_HRTF, "oalgpu_source_params_host: HRTF context without a data set");
        const std::string err = ParseMhr(mhr, mhr_size, hrtf);
        if(!err.empty()) return Fail(OALGPU_ERR_INVALID, "mhr: " + err);
        ResampleHrtfData(hrtf, desc->sample_rate);
        store = HostStoreView(hrtf);
    }
    const ResamplerConsts &rs = HostResamplerConsts();
    const SourceSetup cx{desc->sample_rate, desc->num_aux_sends, numSlots, numDry, wet, desc->hrtf ? 1u : 0u, env.data(), &rs,
        dryMap.data(), wetMaps.data()};
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_source_props &p = props[i];
        if(!PropsOk(p, cx.numSends, numSlots)) return Fail(OALGPU_ERR_INVALID, "oalgpu_source_params_host: resampler, distance model or send slot out of range");
        oalgpu_voice_params &o = out[i];
        std::memset(&o, 0, sizeof(o));
        const SourceGains g = SourceAttenuation(p, frequency, *listener, cx);
        const uint32_t flags = SourceFilterFlags(g, cx.numSends);
        o.step = g.step;
        o.resampler = p.resampler;
        const float invSampleRate = 1.0f / float(cx.sampleRate);
        o.direct_filter = oalgpu_filter_params{(flags & kFlagDirectFilter) ? 1 : 0, g.dryHF, p.direct_hf_reference * invSampleRate,
            g.dryLF, p.direct_lf_reference * invSampleRate};
        o.hrtf_ev = g.hrtfEv; o.hrtf_az = g.hrtfAz; o.hrtf_dist = g.hrtfDist; o.hrtf_spread = g.spread;
        o.hrtf_gain = g.dryBase;
        const float ay = -g.dir[0], az = g.dir[1], ax = -g.dir[2];
        if(!cx.hrtf)
            for(uint32_t t = 0; t < numDry; ++t)
                o.dry_gains[t] = PanLineGain(dryMap[t].index, dryMap[t].scale, ay, az, ax, g.spread, g.dryBase);
        for(uint32_t s = 0; s < OALGPU_MAX_SENDS; ++s)
        {
            o.send_slot[s] = g.sendSlot[s];
            if(s >= cx.numSends) continue;
            o.send_filter[s] = oalgpu_filter_params{(flags >> (kFlagSendFilterShift + s)) & 1u ? 1 : 0, g.wetHF[s],
                p.send[s].hf_reference * invSampleRate, g.wetLF[s], p.send[s].lf_reference * invSampleRate};
            if(g.sendSlot[s] < 0) continue;
            for(uint32_t ch = 0; ch < wet; ++ch)
            {
                const AmbiMapEntry &m = wetMaps[size_t(g.sendSlot[s]) * wet + ch];
                o.send_gains[s][ch] = PanLineGain(m.index, m.scale, ay, az, ax, g.spread, g.wetBase[s]);
            }
        }
    }
    return OALGPU_OK;
}
