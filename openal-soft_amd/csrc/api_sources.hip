// Source parameters computed on the GPU: the listener, the slots' send environments, and the entry points that turn source
// properties into parameter records.  Three kinds of source, each with a collector (what the call refuses; the kind's records
// and the voices in output order), a params kernel and the same arithmetic compiled for the host:
//   mono 3D sources      CollectSources          SourceParamsKernel (source_kernels.hip)           dev_source.hpp           oalgpu_source_params_host
//   channel sources      CollectChannelSources   ChannelParamsKernel (source_channel_kernels.hip)  dev_source_channels.hpp  oalgpu_channel_source_params_host
//   ambisonic sources    CollectAmbiSources      AmbiParamsKernel (source_ambi_kernels.hip)        dev_source_ambi.hpp      oalgpu_ambi_source_params_host
// Behind the collector every entry point is one of two paths over the kind's launch: ApplyCollected (the synchronous call) or
// BlockFromCollected (a parameter block).  On a context with near-field control that knows its speaker distance the first two
// kinds' launches also run the near-field side: SourceNfcKernel and ApplyNfcKernel (source_nfc_kernels.hip), dev_source_nfc.hpp,
// oalgpu_channel_source_nfc_host.
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

// ---- the collectors: what a call refuses, and of what it accepts the kind's source records (c->srcHost, c->chanHost or
// c->ambiHost, with their places in the output) and the voices in output order (c->srcVoices) ----

// the contexts the pan-gain kinds refuse
int StageContextOk(const oalgpu_context *c, const std::string &name)
{
    if(c->L.hrtf && !c->hrtfLoaded) return Fail(OALGPU_ERR_NO_HRTF, name + ": HRTF context without a data set");
    if(c->L.nfc && !(c->nfcAvgDist > 0.0f))
        return Fail(OALGPU_ERR_INVALID, name + ": not for contexts with near-field control whose speaker distance is not set (oalgpu_context_set_nfc_distance; without it the per-voice w0 adjust stays with the host: oalgpu_voice_set_nfc)");
    return OALGPU_OK;
}

bool ChannelSourceOk(const oalgpu_channel_source &src)
{
    return src.channels >= OALGPU_CHANNELS_MONO && src.channels <= OALGPU_CHANNELS_X71 && src.spatialize >= OALGPU_SPATIALIZE_OFF
        && src.spatialize <= OALGPU_SPATIALIZE_AUTO;
}

// one channel voice of a multi-channel source: what is refused of it; otherwise it is named, `frequency` (0: the source's
// first voice) is the source's, and the voice is next in the output
int ClaimChannelVoice(oalgpu_context *c, const std::string &name, uint32_t v, std::vector<uint8_t> &named, uint32_t &frequency)
{
    if(v >= c->L.numVoices) return Fail(OALGPU_ERR_INVALID, name + ": bad voice index");
    if(c->cbOfVoice[v] >= 0)
        return Fail(OALGPU_ERR_INVALID, name + ": not for callback voices (their step is mirrored on the host: oalgpu_voice_set_params)");
    if(named[v]) return Fail(OALGPU_ERR_INVALID, name + ": a voice named twice");
    named[v] = 1;
    const uint32_t freq = v < c->voiceFreq.size() ? c->voiceFreq[v] : 0u;
    if(freq == 0u) return Fail(OALGPU_ERR_INVALID, name + ": the voice has no frequency (start it with oalgpu_voice_init)");
    if(frequency && frequency != freq)
        return Fail(OALGPU_ERR_INVALID, name + ": the channel voices of a source have different frequencies");
    frequency = freq;
    c->srcVoices.push_back(v);
    return OALGPU_OK;
}

int CollectSources(oalgpu_context *c, const char *who, const uint32_t *voices, const oalgpu_source_props *props, size_t count)
{
    const std::string name(who);
    if(int rc = StageContextOk(c, name)) return rc;
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

int CollectChannelSources(oalgpu_context *c, const char *who, const oalgpu_channel_source *sources, size_t count)
{
    const std::string name(who);
    if(int rc = StageContextOk(c, name)) return rc;
    std::vector<uint8_t> named(c->L.numVoices, 0);
    c->chanHost.clear(); c->srcVoices.clear();
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_channel_source &src = sources[i];
        if(!ChannelSourceOk(src)) return Fail(OALGPU_ERR_INVALID, name + ": channels or spatialize out of range");
        if(!PropsOk(src.props, c->L.numSends, c->L.numSlots))
            return Fail(OALGPU_ERR_INVALID, name + ": resampler, distance model or send slot out of range");
        ChannelSourceRecord rec{};
        rec.outBase = uint32_t(c->srcVoices.size());
        rec.channels = src.channels; rec.spatialize = src.spatialize;
        rec.stereoPan[0] = src.stereo_pan[0]; rec.stereoPan[1] = src.stereo_pan[1]; rec.panning = src.panning;
        rec.p = src.props;
        for(uint32_t ch = 0; ch < OALGPU_MAX_SOURCE_CHANNELS; ++ch) rec.voices[ch] = OALGPU_NO_VOICE;
        for(uint32_t ch = 0; ch < SourceChannelCount(src.channels); ++ch)
        {
            const uint32_t v = src.voices[ch];
            if(v == OALGPU_NO_VOICE) continue;
            if(int rc = ClaimChannelVoice(c, name, v, named, rec.frequency)) return rc;
            rec.voices[ch] = v;
            rec.present |= 1u << ch;
        }
        if(!rec.frequency) return Fail(OALGPU_ERR_INVALID, name + ": a source without a channel voice");
        c->chanHost.push_back(rec);
    }
    return OALGPU_OK;
}

// a context as oalgpu_source_params_host and oalgpu_channel_source_params_host are told of it: the stage's set-up over host memory
struct HostStage {
    std::vector<oalgpu_slot_environment> env;
    std::vector<AmbiMapEntry> dryMap, wetMaps;
    HrtfData hrtf;
    HrtfStoreDev store{};
    SourceSetup cx{};

    int build(const char *who, const oalgpu_context_desc *desc, const oalgpu_listener_params *listener, const oalgpu_slot_environment *slots,
        const uint8_t *dry_index, const float *dry_scale, const uint8_t *wet_index, const float *wet_scale, const void *mhr,
        size_t mhr_size, uint32_t frequency, bool arraysOk)
    {
        const std::string name(who);
        if(!desc || !listener || !arraysOk || frequency == 0u || desc->sample_rate == 0u)
            return Fail(OALGPU_ERR_INVALID, name + ": bad arguments");
        if(desc->num_aux_sends > OALGPU_MAX_SENDS || desc->num_dry_channels > OALGPU_MAX_OUTPUT_CHANNELS
            || desc->wet_channels > OALGPU_MAX_AMBI_CHANNELS || !dry_index != !dry_scale || !wet_index != !wet_scale)
            return Fail(OALGPU_ERR_INVALID, name + ": bad arguments");
        const uint32_t numDry = desc->num_dry_channels, numSlots = desc->num_slots, wet = desc->wet_channels;
        env.assign(numSlots, oalgpu_slot_environment{0, 0.0f, 0.0f, 1.0f});
        if(slots) std::copy(slots, slots + numSlots, env.begin());
        dryMap.resize(numDry); wetMaps.resize(size_t{numSlots} * wet);
        for(uint32_t i = 0; i < numDry; ++i) dryMap[i] = dry_index ? AmbiMapEntry{dry_index[i], dry_scale[i]} : AmbiMapEntry{i, 1.0f};
        for(size_t i = 0; i < wetMaps.size(); ++i)
            wetMaps[i] = wet_index ? AmbiMapEntry{wet_index[i], wet_scale[i]} : AmbiMapEntry{uint32_t(i % wet), 1.0f};
        for(const AmbiMapEntry &m : dryMap) if(m.index >= OALGPU_MAX_AMBI_CHANNELS) return Fail(OALGPU_ERR_INVALID, "ambisonic channel index out of range");
        for(const AmbiMapEntry &m : wetMaps) if(m.index >= OALGPU_MAX_AMBI_CHANNELS) return Fail(OALGPU_ERR_INVALID, "ambisonic channel index out of range");
        if(desc->hrtf)
        {
            if(!mhr) return Fail(OALGPU_ERR_NO_HRTF, name + ": HRTF context without a data set");
            const std::string err = ParseMhr(mhr, mhr_size, hrtf);
            if(!err.empty()) return Fail(OALGPU_ERR_INVALID, "mhr: " + err);
            ResampleHrtfData(hrtf, desc->sample_rate);
            store = HostStoreView(hrtf);
        }
        cx = SourceSetup{desc->sample_rate, desc->num_aux_sends, numSlots, numDry, wet, desc->hrtf ? 1u : 0u, env.data(),
            &HostResamplerConsts(), dryMap.data(), wetMaps.data()};
        return OALGPU_OK;
    }
};

// what the stage leaves for one voice whatever pans it, as an oalgpu_voice_params cleared otherwise: the step, the resampler,
// the filters' parameters in place of the designs, the send slots
void FillVoiceCommon(oalgpu_voice_params &o, const oalgpu_source_props &p, const SourceGains &g, const SourceSetup &cx)
{
    std::memset(&o, 0, sizeof(o));
    const uint32_t flags = SourceFilterFlags(g, cx.numSends);
    o.step = g.step;
    o.resampler = p.resampler;
    const float invSampleRate = 1.0f / float(cx.sampleRate);
    o.direct_filter = oalgpu_filter_params{(flags & kFlagDirectFilter) ? 1 : 0, g.dryHF, p.direct_hf_reference * invSampleRate,
        g.dryLF, p.direct_lf_reference * invSampleRate};
    for(uint32_t s = 0; s < OALGPU_MAX_SENDS; ++s)
    {
        o.send_slot[s] = g.sendSlot[s];
        if(s < cx.numSends)
            o.send_filter[s] = oalgpu_filter_params{(flags >> (kFlagSendFilterShift + s)) & 1u ? 1 : 0, g.wetHF[s],
                p.send[s].hf_reference * invSampleRate, g.wetLF[s], p.send[s].lf_reference * invSampleRate};
    }
}

// the same with the resolved line gains of a voice panned by a direction
void FillVoiceParams(oalgpu_voice_params &o, const oalgpu_source_props &p, const SourceGains &g, const ChannelPan &pan, const HostStage &h)
{
    const SourceSetup &cx = h.cx;
    FillVoiceCommon(o, p, g, cx);
    o.hrtf_ev = pan.hrtfEv; o.hrtf_az = pan.hrtfAz; o.hrtf_dist = pan.hrtfDist; o.hrtf_spread = pan.hrtfSpread;
    const float dryGain = g.dryBase * pan.pangain;
    o.hrtf_gain = dryGain;
    const float ay = -pan.dir[0], az = pan.dir[1], ax = -pan.dir[2];
    if(!cx.hrtf && !pan.silent)
        for(uint32_t t = 0; t < cx.numDry; ++t)
            o.dry_gains[t] = PanLineGain(h.dryMap[t].index, h.dryMap[t].scale, ay, az, ax, pan.drySpread, dryGain);
    for(uint32_t s = 0; s < cx.numSends; ++s)
    {
        if(g.sendSlot[s] < 0 || pan.silent) continue;
        for(uint32_t ch = 0; ch < cx.wetChannels; ++ch)
        {
            const AmbiMapEntry &m = h.wetMaps[size_t(g.sendSlot[s]) * cx.wetChannels + ch];
            o.send_gains[s][ch] = PanLineGain(m.index, m.scale, ay, az, ax, pan.sendSpread, g.wetBase[s] * pan.pangain);
        }
    }
}

// ---- a collected call on the device.  The collector has left the kind's records and c->srcVoices; the kind's launch -- a
// StageLaunch -- stages the records and launches its params kernel into `out` and, on near-field contexts, SourceNfcKernel over
// the same staged records into `nfcOut`, on the context's stream.  Two consumers: the synchronous call and the block. ----
using StageLaunch = int (*)(oalgpu_context *c, ParamRecord *out, NfcRecord *nfcOut);

int RunNfcStage(oalgpu_context *c, const SourceRecord *mono, const ChannelSourceRecord *chan, size_t sources, NfcRecord *out)
{
    if(!c->L.nfc) return OALGPU_OK;
    LaunchSourceNfc(c->stream, SetupOf(c), c->listener, NfcSetupOf(c), mono, chan, uint32_t(sources), out);
    HIP_TRY(hipGetLastError());
    return OALGPU_OK;
}

int LaunchMonoStage(oalgpu_context *c, ParamRecord *out, NfcRecord *nfcOut)
{
    const size_t count = c->srcHost.size();
    if(int rc = StageRecords(c->stream, c->srcDev, c->srcHost.data(), count)) return rc;
    LaunchSourceParams(c->stream, SetupOf(c), c->hrtfDev, c->listener, c->srcDev.p, uint32_t(count), out);
    HIP_TRY(hipGetLastError());
    return RunNfcStage(c, c->srcDev.p, nullptr, count, nfcOut);
}

int LaunchChannelStage(oalgpu_context *c, ParamRecord *out, NfcRecord *nfcOut)
{
    const size_t count = c->chanHost.size();
    if(int rc = StageRecords(c->stream, c->chanDev, c->chanHost.data(), count)) return rc;
    uint32_t maxChannels = 1;
    for(const ChannelSourceRecord &r : c->chanHost) maxChannels = std::max(maxChannels, SourceChannelCount(r.channels));
    LaunchChannelParams(c->stream, SetupOf(c), c->hrtfDev, c->listener, c->chanDev.p, uint32_t(count), maxChannels, out);
    HIP_TRY(hipGetLastError());
    return RunNfcStage(c, nullptr, c->chanDev.p, count, nfcOut);
}

// the records into c->paramDev / c->nfcRecDev, installed in the voices: params, NFC, apply params, apply NFC, synchronize
int ApplyCollected(oalgpu_context *c, StageLaunch launch)
{
    if(int rc = BeginVoiceCall(c)) return rc;
    if(int rc = EnsureSourceStage(c)) return rc;
    const size_t records = c->srcVoices.size();
    if(c->paramDev.n < records) HIP_TRY(c->paramDev.alloc(records));
    if(c->L.nfc && c->nfcRecDev.n < records) HIP_TRY(c->nfcRecDev.alloc(records));
    if(int rc = launch(c, c->paramDev.p, c->nfcRecDev.p)) return rc;
    LaunchApplyParams(c->stream, c->L, c->paramDev.p, uint32_t(records));
    HIP_TRY(hipGetLastError());
    if(c->L.nfc) { ApplyNfcRecords(c, c->nfcRecDev.p, uint32_t(records)); HIP_TRY(hipGetLastError()); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OALGPU_OK;
}

// the records into a new block
int BlockFromCollected(oalgpu_context *c, StageLaunch launch, oalgpu_param_block **out)
{
    if(int rc = UseCtx(c)) return rc;
    if(int rc = EnsureSourceStage(c)) return rc;
    const size_t records = c->srcVoices.size();
    auto b = std::make_unique<oalgpu_param_block>();
    b->count = uint32_t(records);
    b->device = c->desc.device;
    b->hrtfGeneration = c->hrtfGeneration;
    HIP_TRY(b->recs.alloc(records));
    if(c->L.nfc) HIP_TRY(b->nfc.alloc(records));
    if(int rc = launch(c, b->recs.p, b->nfc.p)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));       // (the staging is free again; the rows below read finished records)
    if(int rc = FinishParamBlock(c, b.get(), c->srcVoices.data(), records)) return rc;
    *out = b.release();
    return OALGPU_OK;
}

} // namespace

NfcSetup NfcSetupOf(const oalgpu_context *c)
{
    const NfcDesign &d = c->nfcDevice;
    return NfcSetup{c->nfcAvgDist, {d.baseGain[1], d.baseGain[2], d.baseGain[3], d.baseGain[4]}};
}

void ApplyNfcRecords(oalgpu_context *c, const NfcRecord *recs, uint32_t count)
{
    NfcDeviceCoeffs a{};
    for(uint32_t o = 1; o <= 4u; ++o)
        for(uint32_t k = 1; k <= o; ++k) a.a[NfcPacked(o, k)] = c->nfcDevice.a[o][k];
    LaunchApplyNfc(c->stream, c->L, a, recs, count);
}

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
    return ApplyCollected(c, LaunchMonoStage);
}

int oalgpu_param_block_create_from_sources(oalgpu_context *c, const uint32_t *voices, const oalgpu_source_props *props, size_t count,
    oalgpu_param_block **out)
{
    if(!c || !voices || !props || !out || count == 0)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_param_block_create_from_sources: bad arguments");
    *out = nullptr;
    if(int rc = CollectSources(c, "oalgpu_param_block_create_from_sources", voices, props, count)) return rc;
    return BlockFromCollected(c, LaunchMonoStage, out);
}

int oalgpu_source_params_host(const oalgpu_context_desc *desc, const oalgpu_listener_params *listener,
    const oalgpu_slot_environment *slots, const uint8_t *dry_index, const float *dry_scale, const uint8_t *wet_index,
    const float *wet_scale, const void *mhr, size_t mhr_size, uint32_t frequency, const oalgpu_source_props *props, size_t count,
    oalgpu_voice_params *out)
{
    HostStage h;
    if(int rc = h.build("oalgpu_source_params_host", desc, listener, slots, dry_index, dry_scale, wet_index, wet_scale, mhr, mhr_size,
        frequency, props && out))
        return rc;
    const float frontPan[2] = {0.0f, 0.0f};
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_source_props &p = props[i];
        if(!PropsOk(p, h.cx.numSends, h.cx.numSlots)) return Fail(OALGPU_ERR_INVALID, "oalgpu_source_params_host: resampler, distance model or send slot out of range");
        const SourceGains g = SourceAttenuation(p, frequency, *listener, h.cx);
        FillVoiceParams(out[i], p, g, ChannelPanning(ChannelSeatOf(OALGPU_CHANNELS_MONO, 0u, frontPan, 0.0f), g, h.cx.hrtf), h);
    }
    return OALGPU_OK;
}

int oalgpu_voice_set_channel_sources(oalgpu_context *c, const oalgpu_channel_source *sources, size_t count)
{
    if(!c || !sources) return Fail(OALGPU_ERR_INVALID, "oalgpu_voice_set_channel_sources: null argument");
    if(count == 0) return OALGPU_OK;
    if(int rc = CollectChannelSources(c, "oalgpu_voice_set_channel_sources", sources, count)) return rc;
    return ApplyCollected(c, LaunchChannelStage);
}

int oalgpu_param_block_create_from_channel_sources(oalgpu_context *c, const oalgpu_channel_source *sources, size_t count,
    oalgpu_param_block **out)
{
    if(!c || !sources || !out || count == 0)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_param_block_create_from_channel_sources: bad arguments");
    *out = nullptr;
    if(int rc = CollectChannelSources(c, "oalgpu_param_block_create_from_channel_sources", sources, count)) return rc;
    return BlockFromCollected(c, LaunchChannelStage, out);
}

int oalgpu_channel_source_params_host(const oalgpu_context_desc *desc, const oalgpu_listener_params *listener,
    const oalgpu_slot_environment *slots, const uint8_t *dry_index, const float *dry_scale, const uint8_t *wet_index,
    const float *wet_scale, const void *mhr, size_t mhr_size, uint32_t frequency, const oalgpu_channel_source *sources, size_t count,
    oalgpu_voice_params *out)
{
    HostStage h;
    if(int rc = h.build("oalgpu_channel_source_params_host", desc, listener, slots, dry_index, dry_scale, wet_index, wet_scale, mhr,
        mhr_size, frequency, sources && out))
        return rc;
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_channel_source &src = sources[i];
        if(!ChannelSourceOk(src)) return Fail(OALGPU_ERR_INVALID, "oalgpu_channel_source_params_host: channels or spatialize out of range");
        if(!PropsOk(src.props, h.cx.numSends, h.cx.numSlots))
            return Fail(OALGPU_ERR_INVALID, "oalgpu_channel_source_params_host: resampler, distance model or send slot out of range");
    }
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_channel_source &src = sources[i];
        const SourceGains g = SourceRoute(src.channels, src.spatialize) ? SourceAttenuation(src.props, frequency, *listener, h.cx)
            : SourceNonAttenuation(src.props, frequency, *listener, h.cx);
        const float stereoPan[2] = {src.stereo_pan[0], src.stereo_pan[1]};
        for(uint32_t ch = 0; ch < OALGPU_MAX_SOURCE_CHANNELS; ++ch)
        {
            oalgpu_voice_params &o = out[i * OALGPU_MAX_SOURCE_CHANNELS + ch];
            if(ch >= SourceChannelCount(src.channels)) std::memset(&o, 0, sizeof(o));
            else FillVoiceParams(o, src.props, g, ChannelPanning(ChannelSeatOf(src.channels, ch, stereoPan, src.panning), g, h.cx.hrtf), h);
        }
    }
    return OALGPU_OK;
}

int oalgpu_channel_source_nfc_host(const oalgpu_context_desc *desc, const oalgpu_listener_params *listener,
    const oalgpu_slot_environment *slots, float avg_speaker_dist, uint32_t frequency, const oalgpu_channel_source *sources,
    size_t count, float *w0, float *coeffs)
{
    HostStage h;
    if(int rc = h.build("oalgpu_channel_source_nfc_host", desc, listener, slots, nullptr, nullptr, nullptr, nullptr, nullptr, 0, frequency,
        sources && w0 && coeffs && avg_speaker_dist > 0.0f && desc && !desc->hrtf))
        return rc;
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_channel_source &src = sources[i];
        if(!ChannelSourceOk(src)) return Fail(OALGPU_ERR_INVALID, "oalgpu_channel_source_nfc_host: channels or spatialize out of range");
        if(!PropsOk(src.props, h.cx.numSends, h.cx.numSlots))
            return Fail(OALGPU_ERR_INVALID, "oalgpu_channel_source_nfc_host: resampler, distance model or send slot out of range");
    }
    NfcDesign device;
    NfcInit(343.3f / avg_speaker_dist / float(desc->sample_rate), device);        // InitNearFieldCtrl's w1, in its operation order
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_channel_source &src = sources[i];
        const float distance = SourceRoute(src.channels, src.spatialize) ? SourceAttenuation(src.props, frequency, *listener, h.cx).distance : 0.0f;
        w0[i] = SourceNfcW0(distance, listener->nfc_scale, avg_speaker_dist, desc->sample_rate);
        float *o = coeffs + i * 14;
        for(uint32_t order = 1; order <= 4u; ++order)
        {
            float b[5];
            o[order - 1u] = device.baseGain[order] * NfcOrderDesign(order, w0[i], b);
            for(uint32_t k = 1; k <= order; ++k) o[4u + NfcPacked(order, k)] = b[k];
        }
    }
    return OALGPU_OK;
}

// ---- ambisonic sources (dev_source_ambi.hpp, source_ambi_kernels.hip) ----
namespace {

// RotatorCoeffArray as dev_source_ambi.hpp's FillAmbiRotatorCoeffs computes it, once, at library start
const float *AmbiRotatorCoeffs()
{
    static const std::vector<float> k = [] {
        std::vector<float> r(size_t{kRotatorCoeffs} * 3u);
        FillAmbiRotatorCoeffs(r.data());
        return r;
    }();
    return k.data();
}

// AmbiScale::FromFuMa / FromSN3D / FromN3D (core/ambidefs.h:49-126) from their definitions: N3D is the unit, SN3D -> N3D is
// sqrt(2l + 1), FuMa -> N3D the published maxN weights with W's extra -3 dB (orders 0..3; 1 above)
float AmbiScaleOf(int32_t scaling, uint32_t acn)
{
    const uint32_t l = acn == 0u ? 0u : (acn < 4u ? 1u : (acn < 9u ? 2u : (acn < 16u ? 3u : 4u)));
    if(scaling == OALGPU_AMBI_SCALING_N3D) return 1.0f;
    if(scaling == OALGPU_AMBI_SCALING_SN3D) return float(std::sqrt(double(2u * l + 1u)));
    if(l > OALGPU_MAX_FUMA_ORDER) return 1.0f;
    const double s15 = std::sqrt(15.0) / 2.0, q = std::sqrt(35.0 / 8.0), o = std::sqrt(35.0) / 3.0, m = std::sqrt(224.0 / 45.0);
    const double fuma[16] = {std::sqrt(2.0), std::sqrt(3.0), std::sqrt(3.0), std::sqrt(3.0), s15, s15, std::sqrt(5.0), s15, s15,
        q, o, m, std::sqrt(7.0), m, o, q};
    return float(fuma[acn]);
}

// AmbiIndex::FromFuMa / FromFuMa2D / FromACN / FromACN2D (core/ambidefs.h:143-190): channel c of the buffer -> ACN.  FuMa's
// channel order is W X Y Z R S T U V K L M N O P Q (2D: W X Y U V P Q); ACN's 2D subset is the +-l entry of every band
uint32_t AmbiIndexOf(int32_t layout, bool is2d, uint32_t c)
{
    static const uint8_t fuma[16] = {0, 3, 1, 2, 6, 7, 5, 8, 4, 12, 13, 11, 14, 10, 15, 9};
    static const uint8_t fuma2d[7] = {0, 3, 1, 8, 4, 15, 9};
    if(layout == OALGPU_AMBI_LAYOUT_FUMA) return is2d ? (c < 7u ? fuma2d[c] : 0u) : (c < 16u ? fuma[c] : 0u);
    if(!is2d) return c < kAmbiMax ? c : 0u;
    if(c == 0u) return 0u;
    if(c >= 9u) return 0u;
    const uint32_t l = (c + 1u) / 2u;                       // channels 2l - 1 and 2l are ACN l(l + 1) - l and l(l + 1) + l
    return (c & 1u) ? l * l : l * l + 2u * l;
}

uint32_t AmbiSourceChannels(uint32_t order, bool is2d) { return is2d ? 2u * order + 1u : AmbiChannelsOfOrder(order); }

// what CalcAmbisonicPanning's upsample condition (alu.cpp:1009-1010) makes of a source on a device
bool AmbiNeedsUpsampler(uint32_t deviceOrder, bool mix2d, uint32_t order, bool is2d)
{
    return deviceOrder > order || (deviceOrder >= 2u && !mix2d && is2d);
}

// what the ambisonic entry points refuse of one source besides its voices, and the record's share that does not depend on them
// (upsampler: the source's, null = not given; the record's upOffset is the caller's)
int AmbiSourceHead(const std::string &name, const oalgpu_ambi_source &src, uint32_t deviceOrder, bool mix2d, bool upGiven,
    uint32_t numSends, uint32_t numSlots, AmbiSourceRecord &rec)
{
    if(src.spatialize < OALGPU_SPATIALIZE_OFF || src.spatialize > OALGPU_SPATIALIZE_AUTO || src.order < 1u || src.order > OALGPU_MAX_AMBI_ORDER
        || src.layout < OALGPU_AMBI_LAYOUT_FUMA || src.layout > OALGPU_AMBI_LAYOUT_ACN || src.scaling < OALGPU_AMBI_SCALING_FUMA
        || src.scaling > OALGPU_AMBI_SCALING_N3D)
        return Fail(OALGPU_ERR_INVALID, name + ": spatialize, order, layout or scaling out of range");
    if((src.layout == OALGPU_AMBI_LAYOUT_FUMA || src.scaling == OALGPU_AMBI_SCALING_FUMA) && src.order > OALGPU_MAX_FUMA_ORDER)
        return Fail(OALGPU_ERR_INVALID, name + ": FuMa layout and scaling reach order 3 (AmbiIndex::FromFuMa, AmbiScale::FromFuMa)");
    if(!PropsOk(src.props, numSends, numSlots))
        return Fail(OALGPU_ERR_INVALID, name + ": resampler, distance model or send slot out of range");
    const bool is2d = src.is_2d != 0;
    const bool upsample = AmbiNeedsUpsampler(deviceOrder, mix2d, src.order, is2d);
    if(upsample && !upGiven)
        return Fail(OALGPU_ERR_INVALID, name + ": the source needs an upsampler the context has not been given (oalgpu_context_set_ambi_upsampler)");
    rec = AmbiSourceRecord{};
    rec.spatialize = src.spatialize;
    rec.channels = AmbiSourceChannels(src.order, is2d);
    rec.upRows = upsample ? AmbiChannelsOfOrder(src.order) : 0u;
    rec.scale0 = AmbiScaleOf(src.scaling, 0u);
    for(int k = 0; k < 3; ++k) { rec.orientAt[k] = src.orient_at[k]; rec.orientUp[k] = src.orient_up[k]; }
    for(uint32_t ch = 0; ch < kAmbiMax; ++ch)
    {
        const uint32_t acn = ch < rec.channels ? AmbiIndexOf(src.layout, is2d, ch) : 0u;
        rec.acn[ch] = uint8_t(acn);
        rec.scale[ch] = AmbiScaleOf(src.scaling, acn);
        rec.voices[ch] = OALGPU_NO_VOICE;
    }
    rec.p = src.props;
    return OALGPU_OK;
}

uint32_t AmbiUpSlot(uint32_t order, bool is2d) { return (order - 1u) * 2u + (is2d ? 1u : 0u); }

// CollectChannelSources for ambisonic sources: the records (c->ambiHost) and the voices in output order (c->srcVoices)
int CollectAmbiSources(oalgpu_context *c, const char *who, const oalgpu_ambi_source *sources, size_t count)
{
    const std::string name(who);
    if(c->L.hrtf)
        return Fail(OALGPU_ERR_INVALID, name + ": not for HRTF contexts (their voice kernels mix only through the FIR; B-Format voices need dry lines)");
    if(!c->ambiOrder) return Fail(OALGPU_ERR_INVALID, name + ": the context has not been told its ambisonic order (oalgpu_context_set_ambi_order)");
    if(c->L.nfc)
        return Fail(OALGPU_ERR_INVALID, name + ": not for contexts with near-field control (B-Format voices keep the per-voice adjust: oalgpu_voice_set_nfc)");
    std::vector<uint8_t> named(c->L.numVoices, 0);
    c->ambiHost.clear(); c->srcVoices.clear();
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_ambi_source &src = sources[i];
        AmbiSourceRecord rec;
        const bool inRange = src.order >= 1u && src.order <= OALGPU_MAX_AMBI_ORDER;
        const uint32_t slot = inRange ? AmbiUpSlot(src.order, src.is_2d != 0) : 0u;
        if(int rc = AmbiSourceHead(name, src, c->ambiOrder, c->ambiMix2d, c->ambiUpGiven[slot], c->L.numSends, c->L.numSlots, rec)) return rc;
        rec.upOffset = slot * kAmbiMatrix;
        rec.outBase = uint32_t(c->srcVoices.size());
        for(uint32_t ch = 0; ch < rec.channels; ++ch)
        {
            const uint32_t v = src.voices[ch];
            if(v == OALGPU_NO_VOICE) continue;
            if(int rc = ClaimChannelVoice(c, name, v, named, rec.frequency)) return rc;
            rec.voices[ch] = v;
            rec.present |= 1u << ch;
        }
        if(!rec.frequency) return Fail(OALGPU_ERR_INVALID, name + ": a source without a channel voice");
        c->ambiHost.push_back(rec);
    }
    return OALGPU_OK;
}

// the device side of the ambisonic stage, allocated with its first use
int EnsureAmbiStage(oalgpu_context *c)
{
    if(!c->ambiRotDev.p)
    {
        HIP_TRY(c->ambiRotDev.alloc(size_t{kRotatorCoeffs} * 3u));
        HIP_TRY(c->ambiRotDev.upload(AmbiRotatorCoeffs(), size_t{kRotatorCoeffs} * 3u));
    }
    if(!c->ambiUpDev.p)
    {
        c->ambiUpHost.resize(size_t{8} * kAmbiMatrix, 0.0f);
        HIP_TRY(c->ambiUpDev.alloc(c->ambiUpHost.size()));
        HIP_TRY(c->ambiUpDev.upload(c->ambiUpHost.data(), c->ambiUpHost.size()));
    }
    return OALGPU_OK;
}

// the ambisonic kind's StageLaunch (no near-field side: the collector refuses those contexts)
int LaunchAmbiStage(oalgpu_context *c, ParamRecord *out, NfcRecord *)
{
    if(int rc = EnsureAmbiStage(c)) return rc;
    if(int rc = StageRecords(c->stream, c->ambiDev, c->ambiHost.data(), c->ambiHost.size())) return rc;
    LaunchAmbiParams(c->stream, SetupOf(c), AmbiSetup{c->ambiOrder, c->ambiRotDev.p, c->ambiUpDev.p}, c->listener, c->ambiDev.p,
        uint32_t(c->ambiHost.size()), out);
    HIP_TRY(hipGetLastError());
    return OALGPU_OK;
}

} // namespace

int oalgpu_context_set_ambi_order(oalgpu_context *c, uint32_t order, int32_t mix_2d)
{
    if(!c || order < 1u || order > OALGPU_MAX_AMBI_ORDER) return Fail(OALGPU_ERR_INVALID, "oalgpu_context_set_ambi_order: bad arguments");
    if(int rc = BeginVoiceCall(c, true, "", true)) return rc;      // (no source launch in flight reads it)
    c->ambiOrder = order; c->ambiMix2d = mix_2d != 0;
    return OALGPU_OK;
}

int oalgpu_context_set_ambi_upsampler(oalgpu_context *c, uint32_t source_order, int32_t is_2d, const float *matrix, uint32_t rows)
{
    if(!c || !matrix || source_order < 1u || source_order > OALGPU_MAX_AMBI_ORDER || rows != AmbiChannelsOfOrder(source_order))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_context_set_ambi_upsampler: bad arguments (rows = (source_order + 1)^2)");
    if(int rc = BeginVoiceCall(c, true, "", true)) return rc;      // (no source launch in flight reads the store)
    if(int rc = EnsureAmbiStage(c)) return rc;
    const uint32_t slot = AmbiUpSlot(source_order, is_2d != 0);
    float *host = c->ambiUpHost.data() + size_t{slot} * kAmbiMatrix;
    std::fill(host, host + kAmbiMatrix, 0.0f);
    std::copy(matrix, matrix + size_t{rows} * kAmbiMax, host);
    HIP_TRY(hipMemcpy(c->ambiUpDev.p + size_t{slot} * kAmbiMatrix, host, kAmbiMatrix * sizeof(float), hipMemcpyHostToDevice));
    c->ambiUpGiven[slot] = true;
    return OALGPU_OK;
}

int oalgpu_voice_set_ambi_sources(oalgpu_context *c, const oalgpu_ambi_source *sources, size_t count)
{
    if(!c || !sources) return Fail(OALGPU_ERR_INVALID, "oalgpu_voice_set_ambi_sources: null argument");
    if(count == 0) return OALGPU_OK;
    if(int rc = CollectAmbiSources(c, "oalgpu_voice_set_ambi_sources", sources, count)) return rc;
    return ApplyCollected(c, LaunchAmbiStage);
}

int oalgpu_param_block_create_from_ambi_sources(oalgpu_context *c, const oalgpu_ambi_source *sources, size_t count,
    oalgpu_param_block **out)
{
    if(!c || !sources || !out || count == 0)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_param_block_create_from_ambi_sources: bad arguments");
    *out = nullptr;
    if(int rc = CollectAmbiSources(c, "oalgpu_param_block_create_from_ambi_sources", sources, count)) return rc;
    return BlockFromCollected(c, LaunchAmbiStage, out);
}

int oalgpu_ambi_source_params_host(const oalgpu_context_desc *desc, const oalgpu_listener_params *listener,
    const oalgpu_slot_environment *slots, const uint8_t *dry_index, const float *dry_scale, const uint8_t *wet_index,
    const float *wet_scale, const oalgpu_ambi_device *device, uint32_t frequency, const oalgpu_ambi_source *sources, size_t count,
    oalgpu_voice_params *out, float *rot_out, float *mix_out)
{
    const std::string name("oalgpu_ambi_source_params_host");
    HostStage h;
    if(int rc = h.build("oalgpu_ambi_source_params_host", desc, listener, slots, dry_index, dry_scale, wet_index, wet_scale, nullptr, 0,
        frequency, sources && out && device && desc && !desc->hrtf && device->order >= 1u && device->order <= OALGPU_MAX_AMBI_ORDER))
        return rc;
    const SourceSetup &cx = h.cx;
    std::vector<AmbiSourceRecord> recs(count);
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_ambi_source &src = sources[i];
        const bool inRange = src.order >= 1u && src.order <= OALGPU_MAX_AMBI_ORDER;
        const bool given = inRange && device->upsampler[src.order - 1u][src.is_2d ? 1 : 0] != nullptr;
        if(int rc = AmbiSourceHead(name, src, device->order, device->mix_2d != 0, given, cx.numSends, cx.numSlots, recs[i])) return rc;
    }
    const uint32_t devChannels = AmbiChannelsOfOrder(device->order);
    const float *uvwAll = AmbiRotatorCoeffs();
    std::vector<float> rot(kAmbiMatrix), mix(kAmbiMatrix);
    for(size_t i = 0; i < count; ++i)
    {
        const oalgpu_ambi_source &src = sources[i];
        const AmbiSourceRecord &rec = recs[i];
        const oalgpu_source_props &p = rec.p;
        const bool attenuated = AmbiSourceRoute(rec.spatialize);
        const SourceGains g = attenuated ? SourceAttenuation(p, frequency, *listener, cx) : SourceNonAttenuation(p, frequency, *listener, cx);
        const float coverage = AmbiCoverage(g.distance, g.spread);
        const bool covered = coverage > 0.0f;
        float pos[3], panned[kAmbiMax];
        AmbiPanPosition(g, attenuated, pos);
        for(uint32_t j = 0; j < kAmbiMax; ++j) panned[j] = AmbiCoeff(j, -pos[0], pos[1], -pos[2]);
        std::fill(rot.begin(), rot.end(), 0.0f); std::fill(mix.begin(), mix.end(), 0.0f);
        if(covered)
        {
            float block[9];
            AmbiOrientation(rec.orientAt, rec.orientUp, p.head_relative, *listener, block);
            rot[0] = 1.0f;
            for(uint32_t k = 0; k < 9u; ++k) rot[(1u + k / 3u) * kAmbiMax + 1u + k % 3u] = block[k];
            for(uint32_t l = 2; l <= device->order; ++l)
            {
                const uint32_t side = 2u * l + 1u, base = l * l;
                const float *uvw = uvwAll + 3u * AmbiRotatorBandStart(l);
                for(uint32_t e = 0; e < side * side; ++e)
                    rot[(base + e / side) * kAmbiMax + base + e % side]
                        = AmbiRotatorElement(rot.data(), uvw + 3u * e, int(l), int(e / side) - int(l), int(e % side) - int(l));
            }
            if(rec.upRows)
            {
                const float *up = device->upsampler[src.order - 1u][src.is_2d ? 1 : 0];
                for(uint32_t r = 0; r < rec.upRows; ++r)
                    for(uint32_t j = 0; j < kAmbiMax; ++j)
                        mix[r * kAmbiMax + j] = AmbiUpsampleEntry(rot.data(), up + size_t{r} * kAmbiMax, j, devChannels);
            }
            else mix = rot;
        }
        if(rot_out) std::copy(rot.begin(), rot.end(), rot_out + i * kAmbiMatrix);
        if(mix_out) std::copy(mix.begin(), mix.end(), mix_out + i * kAmbiMatrix);

        const float pannedScale = (1.0f - coverage) * rec.scale0;
        for(uint32_t ch = 0; ch < kAmbiMax; ++ch)
        {
            oalgpu_voice_params &o = out[i * kAmbiMax + ch];
            if(ch >= rec.channels) { std::memset(&o, 0, sizeof(o)); continue; }
            FillVoiceCommon(o, p, g, cx);
            const uint32_t row = uint32_t(rec.acn[ch]) * kAmbiMax;
            const float scale = rec.scale[ch] * coverage;
            auto line = [&](const AmbiMapEntry &m, float base) {
                if(covered) return AmbiLineGain(m.scale, AmbiChannelCoeff(mix[row + m.index], scale, ch == 0u ? panned[m.index] * pannedScale : 0.0f), base);
                return ch == 0u ? AmbiLineGain(m.scale, panned[m.index], base * rec.scale0) : 0.0f;
            };
            for(uint32_t t = 0; t < cx.numDry; ++t) o.dry_gains[t] = line(h.dryMap[t], g.dryBase);
            for(uint32_t s = 0; s < cx.numSends; ++s)
            {
                if(g.sendSlot[s] < 0) continue;
                for(uint32_t wc = 0; wc < cx.wetChannels; ++wc)
                    o.send_gains[s][wc] = line(h.wetMaps[size_t(g.sendSlot[s]) * cx.wetChannels + wc], g.wetBase[s]);
            }
        }
    }
    return OALGPU_OK;
}

int oalgpu_ambi_tables_host(float *scales, uint8_t *index)
{
    if(!scales || !index) return Fail(OALGPU_ERR_INVALID, "oalgpu_ambi_tables_host: null argument");
    for(int32_t s = 0; s < 3; ++s)
        for(uint32_t acn = 0; acn < kAmbiMax; ++acn) scales[s * int(kAmbiMax) + int(acn)] = AmbiScaleOf(s, acn);
    for(uint32_t t = 0; t < 4u; ++t)
        for(uint32_t ch = 0; ch < kAmbiMax; ++ch)
            index[t * kAmbiMax + ch] = uint8_t(AmbiIndexOf(t < 2u ? OALGPU_AMBI_LAYOUT_FUMA : OALGPU_AMBI_LAYOUT_ACN, (t & 1u) != 0u, ch));
    return OALGPU_OK;
}
