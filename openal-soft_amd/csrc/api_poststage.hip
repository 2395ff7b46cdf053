// The post stage of a context: what stands between the mixed buses and the output lines.  A non-HRTF context has ONE post-process
// (c->post, the reference's PostProcess variant), then the limiter, then distance compensation; the setters install them and
// RunSpeakerPost runs them.  An HRTF context post-processes with MixDirectHrtf (api.hip) and has the limiter only.
#include "api_context.hpp"

static const char *const kPostNames[6] = {"nothing", "B-Format decoder", "front stabilizer", "crossfeed", "UHJ encoder", "TSME encoder"};

constexpr uint32_t Bit(PostKind k) { return 1u << uint32_t(k); }

// Who may replace whom: [requested kind] -> the installed kinds the request is accepted over.  None is "decoder off": the
// stabilizer and the crossfeed decode with the decoder, so it stays while they do.  A decoder installed over one of the two
// replaces the decoder under it and the kind stays.  Removing any other kind is never refused (RemovePost).
static const uint32_t kAcceptedOver[6] = {
    /* None       */ Bit(PostKind::None) | Bit(PostKind::AmbiDec) | Bit(PostKind::Uhj) | Bit(PostKind::Tsme),
    /* AmbiDec    */ Bit(PostKind::None) | Bit(PostKind::AmbiDec) | Bit(PostKind::Stabilizer) | Bit(PostKind::Bs2b),
    /* Stabilizer */ Bit(PostKind::AmbiDec) | Bit(PostKind::Stabilizer),
    /* Bs2b       */ Bit(PostKind::AmbiDec) | Bit(PostKind::Bs2b),
    /* Uhj        */ Bit(PostKind::None) | Bit(PostKind::Uhj),
    /* Tsme       */ Bit(PostKind::None) | Bit(PostKind::Tsme),
};

// An attached context (oalgpu_context_attach) has no post stage: what the attach refuses to find installed cannot be installed
// afterwards either.  Removals stay open.
static const char kAttachedHasNoPostStage[] = "the context is attached (oalgpu_context_attach): its device context has the post stage";

static int CheckPost(const oalgpu_context *c, const char *who, PostKind want)
{
    const std::string w = std::string(who) + ": ";
    if(c->L.hrtf) return Fail(OALGPU_ERR_INVALID, w + "an HRTF context post-processes with MixDirectHrtf");
    if(c->attachedTo && want != PostKind::None) return Fail(OALGPU_ERR_INVALID, w + kAttachedHasNoPostStage);
    if(kAcceptedOver[uint32_t(want)] & Bit(c->post)) return OALGPU_OK;
    const char *have = kPostNames[uint32_t(c->post)];
    if(want == PostKind::None) return Fail(OALGPU_ERR_INVALID, w + "the context's " + have + " decodes with it (remove that first)");
    if(c->post == PostKind::None) return Fail(OALGPU_ERR_INVALID, w + "needs a B-Format decoder (oalgpu_set_bformat_decoder)");
    return Fail(OALGPU_ERR_INVALID, w + "the context post-processes with its " + have);
}

// Only the installed kind can be removed (a TSME removal leaves a UHJ encoder alone); what decoded under it stays
static void RemovePost(oalgpu_context *c, PostKind kind)
{
    if(c->post != kind) return;
    c->post = (kind == PostKind::Stabilizer || kind == PostKind::Bs2b) ? PostKind::AmbiDec : PostKind::None;
}

/* BFormatDec(inchans = num_dry_channels, coeffs, coeffslf, xover_f0norm), core/bformatdec.cpp:27-58 */
int oalgpu_set_bformat_decoder(oalgpu_context *c, uint32_t num_out, const float *coeffs_hf, const float *coeffs_lf,
    float xover_norm)
{
    static const char who[] = "oalgpu_set_bformat_decoder";
    if(!c) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(c->L.hrtf) return Fail(OALGPU_ERR_INVALID, "oalgpu_set_bformat_decoder: an HRTF context post-processes with MixDirectHrtf");
    if(int rc = UseCtx(c)) return rc;
    if(int rc = oalgpu_sync(c)) return rc;
    const bool on = num_out != 0 && coeffs_hf;
    if(int rc = CheckPost(c, who, on ? PostKind::AmbiDec : PostKind::None)) return rc;
    if(!on) { RemovePost(c, PostKind::AmbiDec); return OALGPU_OK; }
    if(num_out > c->L.numReal || num_out > 32u)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_set_bformat_decoder: more output channels than real output lines");
    if(coeffs_lf && !(xover_norm > 0.0f && xover_norm < 0.5f))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_set_bformat_decoder: a dual-band decoder needs 0 < xover_norm < 0.5");
    const uint32_t nin = c->L.numDry;
    // decoder[j].mGains[out] = coeffs[out][j] (bformatdec.cpp:33-38): stored [dry line][32]
    std::vector<float> hf(size_t{nin} * 32, 0.0f), lf(size_t{nin} * 32, 0.0f);
    for(uint32_t j = 0; j < nin && j < OALGPU_MAX_AMBI_CHANNELS; ++j)
        for(uint32_t o = 0; o < num_out; ++o)
        {
            hf[j * 32 + o] = coeffs_hf[size_t{o} * OALGPU_MAX_AMBI_CHANNELS + j];
            if(coeffs_lf) lf[j * 32 + o] = coeffs_lf[size_t{o} * OALGPU_MAX_AMBI_CHANNELS + j];
        }
    HIP_TRY(c->decGainsHf.alloc(hf.size())); HIP_TRY(c->decGainsHf.upload(hf.data(), hf.size()));
    HIP_TRY(c->decGainsLf.alloc(lf.size())); HIP_TRY(c->decGainsLf.upload(lf.data(), lf.size()));
    HIP_TRY(c->decBands.alloc(size_t{nin} * 2 * kLine)); HIP_TRY(c->decBands.zero());
    std::vector<SplitterState> sp(nin);
    for(auto &s : sp) s = SplitterState{coeffs_lf ? SplitterCoeff(xover_norm) : 0.0f, 0.0f, 0.0f, 0.0f};
    HIP_TRY(c->decSplit.alloc(nin)); HIP_TRY(c->decSplit.upload(sp.data(), nin));
    c->decOut = num_out; c->decDual = coeffs_lf != nullptr;
    if(c->post == PostKind::None) c->post = PostKind::AmbiDec;
    return OALGPU_OK;
}

/* The device's output limiter: Compressor::Create's constants (host/limiter_params.cpp), a fresh state, and from the next update
 * on Compressor::process behind every post-process (RunLimiter) */
int oalgpu_limiter_device_params(uint32_t sample_rate, int sample_type, float dither_depth, oalgpu_limiter_params *out)
{
    if(!out || sample_rate == 0 || sample_type < OALGPU_OUT_I8 || sample_type > OALGPU_OUT_F32 || !(dither_depth >= 0.0f))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_limiter_device_params: bad arguments");
    return LimiterDeviceParams(sample_rate, sample_type, dither_depth, out) ? 1 : 0;
}

uint32_t oalgpu_limiter_look_ahead(const oalgpu_limiter_params *params)
{
    LimiterConsts k{};
    if(!params || !LimiterDerive(*params, &k)) return 0u;
    return k.lookAhead;
}

int oalgpu_set_output_limiter(oalgpu_context *c, const oalgpu_limiter_params *params)
{
    if(int rc = BeginSetter(c, "oalgpu_set_output_limiter")) return rc;
    if(params && c->attachedTo) return Fail(OALGPU_ERR_INVALID, std::string("oalgpu_set_output_limiter: ") + kAttachedHasNoPostStage);
    const uint32_t nlines = RealOutLines(c);
    LimiterConsts k{};
    if(params)
    {
        if(params->num_channels != 0 && params->num_channels != nlines)
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_output_limiter: num_channels is not the context's number of output lines");
        if(!LimiterDerive(*params, &k))
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_output_limiter: bad parameters");
        k.numChans = nlines;
    }
    // the kernels of the updates in flight are through with the old state before it goes
    if(int rc = oalgpu_sync(c)) return rc;
    c->limOn = false;
    if(params)
    {
        std::vector<float> init(LimiterStateFloats(nlines), 0.0f);
        std::fill(init.begin() + kLimiterHoldHistory, init.begin() + kLimiterHoldHistory + kLine, -INFINITY);
        HIP_TRY(c->limState.alloc(init.size()));
        HIP_TRY(c->limState.upload(init.data(), init.size()));
        c->lim = k;
        c->limOn = true;
    }
    if(c->outFloats) c->outRing = RingEligible(c);
    return OALGPU_OK;
}

// Compressor::process behind the update's post-process, on the stream that ran it (alc/alu.cpp:2446)
int RunLimiter(oalgpu_context *c, hipStream_t s, uint32_t samplesToDo)
{
    if(!c->limOn) return OALGPU_OK;
    LaunchLimiter(s, RealOut(c), samplesToDo, c->lim, c->limState.p);
    HIP_TRY(hipGetLastError());
    return OALGPU_OK;
}

/* The stereo encoders (UhjPostProcess, alc/alu.cpp:300-311: dry lines W, X, Y; TsmePostProcess, alc/alu.cpp:314-327: dry lines
 * W, Y, Z, X): the quality's taps (host/uhj_params.cpp; both are the same SegmentedFilter<N>), a fresh state, and from the next
 * update on the encode into the two real output lines.  A negative quality removes the encoder of that kind */
static int SetStereoEncoder(oalgpu_context *c, const char *who, PostKind kind, uint32_t needDry, int quality)
{
    if(int rc = BeginSetter(c, who)) return rc;
    if(quality >= 0)
    {
        if(UhjEncoderDelay(quality) == 0)
            return Fail(OALGPU_ERR_INVALID, std::string(who) + ": not a quality of the " + kPostNames[uint32_t(kind)]);
        if(int rc = CheckPost(c, who, kind)) return rc;
        if(c->L.numDry != needDry || c->L.numReal != 2)
            return Fail(OALGPU_ERR_INVALID, std::string(who) + ": needs " + (needDry == 3 ? "three dry lines (W, X, Y)" : "four dry lines (W, Y, Z, X)")
                + " and two real output lines");
    }
    // the kernels of the updates in flight are through with the old state before it goes
    if(int rc = oalgpu_sync(c)) return rc;
    RemovePost(c, kind);
    if(quality >= 0)
    {
        if(const uint32_t len = UhjFirLength(quality))
        {
            const std::vector<float> taps = UhjFirTaps(len);
            HIP_TRY(c->encTaps.alloc(taps.size()));
            HIP_TRY(c->encTaps.upload(taps.data(), taps.size()));
        }
        HIP_TRY(c->encState.alloc(UhjStateFloats(quality)));
        HIP_TRY(c->encState.zero());
        c->encQuality = quality;
        c->post = kind;
    }
    return OALGPU_OK;
}

uint32_t oalgpu_uhj_encoder_delay(int quality) { return UhjEncoderDelay(quality); }
uint32_t oalgpu_tsme_encoder_delay(int quality) { return UhjEncoderDelay(quality); }       // (TsmeEncoder*::getDelay: the same three)
int oalgpu_set_uhj_encoder(oalgpu_context *c, int quality) { return SetStereoEncoder(c, "oalgpu_set_uhj_encoder", PostKind::Uhj, 3, quality); }
int oalgpu_set_tsme_encoder(oalgpu_context *c, int quality) { return SetStereoEncoder(c, "oalgpu_set_tsme_encoder", PostKind::Tsme, 4, quality); }

/* The front stabilizer (StablizerPostProcess, alc/alu.cpp:329-405; CreateStablizer, alc/panning.cpp:160-172): the constants
 * (host/stabilizer_params.cpp), a fresh state, and from the next update on its two kernels around the decode */
int oalgpu_front_stabilizer_constants(float xover_norm, float *out)
{
    StabilizerConsts k{};
    if(!out || !StabilizerDerive(xover_norm, &k))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_front_stabilizer_constants: needs 0 < xover_norm < 0.5");
    out[0] = k.coeff; out[1] = k.midLf; out[2] = k.midHf; out[3] = k.centerLf; out[4] = k.centerHf;
    return OALGPU_OK;
}

int oalgpu_set_front_stabilizer(oalgpu_context *c, const oalgpu_stabilizer_params *params)
{
    static const char who[] = "oalgpu_set_front_stabilizer";
    if(int rc = BeginSetter(c, who)) return rc;
    StabilizerConsts k{};
    if(params)
    {
        if(int rc = CheckPost(c, who, PostKind::Stabilizer)) return rc;
        const uint32_t nr = c->L.numReal;
        if(nr > 32u || params->left >= nr || params->right >= nr || params->center >= nr || params->left == params->right
            || params->left == params->center || params->right == params->center)
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_front_stabilizer: left, right and center are three different real output lines");
        if(!StabilizerDerive(params->xover_norm, &k))
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_front_stabilizer: needs 0 < xover_norm < 0.5");
    }
    // the kernels of the updates in flight are through with the old state before it goes
    if(int rc = oalgpu_sync(c)) return rc;
    RemovePost(c, PostKind::Stabilizer);
    if(params)
    {
        HIP_TRY(c->stabState.alloc(kStabilizerStateFloats));
        HIP_TRY(c->stabState.zero());
        c->stab = k;
        c->stabLeft = params->left; c->stabRight = params->right; c->stabCenter = params->center;
        c->post = PostKind::Stabilizer;
    }
    return OALGPU_OK;
}

/* The bs2b crossfeed (Bs2bPostProcess, alc/alu.cpp:407-434; bs2b_processor::set_params, core/bs2b.cpp): the level's constants
 * at the context's sample rate (host/crossfeed_params.cpp), a fresh state, and from the next update on its two kernels around
 * the decode */
int oalgpu_crossfeed_constants(int level, uint32_t sample_rate, float *out)
{
    CrossfeedConsts k{};
    if(!out || !CrossfeedDerive(level, sample_rate, &k))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_crossfeed_constants: needs a level of 1 to 6 and a sample rate");
    out[0] = k.a0Lo; out[1] = k.b1Lo; out[2] = k.a0Hi; out[3] = k.a1Hi; out[4] = k.b1Hi;
    return OALGPU_OK;
}

int oalgpu_set_crossfeed(oalgpu_context *c, int level, uint32_t left, uint32_t right)
{
    static const char who[] = "oalgpu_set_crossfeed";
    if(int rc = BeginSetter(c, who)) return rc;
    CrossfeedConsts k{};
    if(level != 0)
    {
        if(!CrossfeedDerive(level, c->desc.sample_rate, &k))
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_crossfeed: not a crossfeed level (1 to 6; 0 removes)");
        if(int rc = CheckPost(c, who, PostKind::Bs2b)) return rc;
        if(left >= c->L.numReal || right >= c->L.numReal || left == right)
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_crossfeed: left and right are two different real output lines");
    }
    // the kernels of the updates in flight are through with the old state before it goes
    if(int rc = oalgpu_sync(c)) return rc;
    RemovePost(c, PostKind::Bs2b);
    if(level != 0)
    {
        HIP_TRY(c->cfState.alloc(kCrossfeedStateFloats));
        HIP_TRY(c->cfState.zero());
        c->cf = k;
        c->cfLeft = left; c->cfRight = right;
        c->post = PostKind::Bs2b;
    }
    return OALGPU_OK;
}

/* Speaker distance compensation (ApplyDistanceComp, alc/alu.cpp:2276-2307; InitDistanceComp, alc/panning.cpp:301-371): per
 * output line a delay and a gain, fresh (zero) delay lines, and from the next update on the kernel behind the limiter */
int oalgpu_distance_comp_from_distances(uint32_t sample_rate, const float *distances, uint32_t n, uint32_t *delays, float *gains)
{
    if(sample_rate == 0 || !distances || !delays || !gains || n == 0 || n > 32u)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_distance_comp_from_distances: bad arguments");
    return DistanceCompDerive(sample_rate, distances, n, delays, gains) ? 1 : 0;
}

int oalgpu_set_distance_comp(oalgpu_context *c, uint32_t n, const uint32_t *delays, const float *gains)
{
    if(int rc = BeginSetter(c, "oalgpu_set_distance_comp")) return rc;
    const bool set = n != 0 && delays && gains;
    if(set)
    {
        if(c->attachedTo) return Fail(OALGPU_ERR_INVALID, std::string("oalgpu_set_distance_comp: ") + kAttachedHasNoPostStage);
        if(c->L.hrtf)
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_distance_comp: an HRTF context has no speaker distances to compensate");
        if(n > RealOutLines(c))
            return Fail(OALGPU_ERR_INVALID, "oalgpu_set_distance_comp: more channels than the context has output lines");
        for(uint32_t i = 0; i < n; ++i)
            if(delays[i] > kDistCompMaxDelay)
                return Fail(OALGPU_ERR_INVALID, "oalgpu_set_distance_comp: a delay of more than 1023 samples");
    }
    // the kernels of the updates in flight are through with the old delay lines before they go
    if(int rc = oalgpu_sync(c)) return rc;
    c->distLines = 0;
    if(set)
    {
        HIP_TRY(c->distDelays.alloc(n)); HIP_TRY(c->distDelays.upload(delays, n));
        HIP_TRY(c->distGains.alloc(n)); HIP_TRY(c->distGains.upload(gains, n));
        HIP_TRY(c->distHist.alloc(size_t{n} * kLine)); HIP_TRY(c->distHist.zero());
        c->distLines = n;
    }
    return OALGPU_OK;
}

/* Everything behind the effect slots of a non-HRTF update, on the stream that runs the post-process: the context's one
 * post-process (DeviceBase::Process, alc/alu.cpp:282-434), Compressor::process, ApplyDistanceComp (alc/alu.cpp:2446-2450).
 * The stabilizer and the crossfeed own the decode: their first kernel moves the direct left / right signal out of the real
 * lines in front of it (alu.cpp:339-348, 416-423), their second works on the decoded feeds and adds it back. */
int RunSpeakerPost(oalgpu_context *c, hipStream_t s, uint32_t samplesToDo)
{
    const DeviceLayout &L = c->L;
    float *real = L.bus + size_t{L.numDry} * kLine;
    const PostKind kind = c->post;
    if(kind == PostKind::Stabilizer)
    {
        LaunchStabilizerSplit(s, real, c->stabLeft, c->stabRight, samplesToDo, c->stabState.p);
        HIP_TRY(hipGetLastError());
    }
    if(kind == PostKind::Bs2b)
    {
        LaunchCrossfeedSplit(s, real, c->cfLeft, c->cfRight, samplesToDo, c->cfState.p);
        HIP_TRY(hipGetLastError());
    }
    if(kind == PostKind::AmbiDec || kind == PostKind::Stabilizer || kind == PostKind::Bs2b)
    {   // AmbiDecPostProcess, alc/alu.cpp:282-287: dry lines -> speaker feeds
        LaunchBFormatDecode(s, c->exact, real, L.bus, c->decSplit.p, c->decBands.p, c->decGainsHf.p,
            c->decDual ? c->decGainsLf.p : nullptr, L.numDry, c->decOut, samplesToDo);
        HIP_TRY(hipGetLastError());
    }
    switch(kind)
    {
    case PostKind::None: case PostKind::AmbiDec: break;
    case PostKind::Stabilizer:      // the band split of the decoded mid, the all-passes, the combine (alu.cpp:353-404)
        LaunchStabilizer(s, real, L.numReal, c->stabLeft, c->stabRight, c->stabCenter, samplesToDo, c->stab, c->stabState.p);
        break;
    case PostKind::Bs2b:            // cross_feed over the decoded left and right lines (alu.cpp:429-433)
        LaunchCrossfeed(s, real, c->cfLeft, c->cfRight, samplesToDo, c->cf, c->cfState.p);
        break;
    case PostKind::Uhj:             // UhjEncoder*::encode: FrontLeft / FrontRight delayed and added to
        LaunchUhjEncode(s, c->encQuality, real, real + kLine, L.bus, L.bus + kLine, L.bus + 2 * kLine, samplesToDo, c->encTaps.p,
            c->encState.p);
        break;
    case PostKind::Tsme:            // TsmeEncoder*::encode: likewise
        LaunchTsmeEncode(s, c->encQuality, real, real + kLine, L.bus, samplesToDo, c->encTaps.p, c->encState.p);
        break;
    }
    HIP_TRY(hipGetLastError());
    if(int rc = RunLimiter(c, s, samplesToDo)) return rc;
    if(c->distLines)
    {   // over the limiter's line set
        LaunchDistanceComp(s, RealOut(c), c->distLines, samplesToDo, c->distDelays.p, c->distGains.p, c->distHist.p);
        HIP_TRY(hipGetLastError());
    }
    return OALGPU_OK;
}
