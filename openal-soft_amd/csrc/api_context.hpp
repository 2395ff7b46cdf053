// The device context and what the C-ABI translation units share (api.hip: context life, the update; api_resident.hip: the
// resident voice kernel's host side; api_attach.hip: several contexts on one device; api_slots.hip: the effect slots; api_comm.hip: the
// sharded update's transports; api_percall.hip: the per-call operators; api_hrtf.hip: HRTF data sets; api_buffers.hip: buffer handles;
// api_voices.hip: voices, parameters; api_sources.hip: 3D source parameters computed on the GPU; api_output.hip: what comes back; api_poststage.hip: what is installed and run behind the buses; api_callback.hip:
// callback sources).  Host logic only; no CPU fallback anywhere.
#pragma once
#include "../../include/oalgpu.h"
#ifdef OALGPU_MEASUREMENT
#include "../../tools/measure/oalgpu_measure.h"
#endif

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>          // types and enums only: the library itself is resolved with dlopen/dlsym
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../host/buffer_table.hpp"
#include "../host/mhr.hpp"
#include "../host/hrtf_build.hpp"
#include "../host/params.hpp"
#include "../host/slot_order.hpp"
#include "../host/tables.hpp"
#include "api_util.hpp"
#include "kernels.hpp"
#include "dev_source_nfc.hpp"
#include "dev_source_ambi.hpp"
#include "bus_merge.hpp"
#include "reverb_dev.hpp"

using namespace oalgpu;


namespace oalgpu {

// One blob with every resampler table: [bsinc12 | bsinc24 | bsinc48 | spline | gaussian]
struct TableBlob {
    std::vector<float> data;
    uint32_t bsincBase[3]{};
    uint32_t cubicBase[2]{};
    TableBlob()
    {
        const int fam[3] = {12, 24, 48};
        for(int i = 0; i < 3; ++i)
        {
            const BsincTable *t = GetBsincTable(fam[i]);
            bsincBase[i] = uint32_t(data.size());
            data.insert(data.end(), t->tab.begin(), t->tab.end());
        }
        for(int i = 0; i < 2; ++i)
        {
            const CubicTable *t = GetCubicTable(i);
            cubicBase[i] = uint32_t(data.size());
            data.insert(data.end(), &t->phase[0][0], &t->phase[0][0] + 256);
        }
    }
    uint32_t filterBase(const oalgpu_interp_state &st) const
    {
        switch(st.kind)
        {
        case 2: return cubicBase[st.table ? 1 : 0];
        case 3: case 4: return bsincBase[st.table == 12 ? 0 : st.table == 24 ? 1 : 2] + st.filter_offset;
        default: return 0;
        }
    }
};
inline const TableBlob &Blob() { static const TableBlob b; return b; }

} // namespace oalgpu

// The post-process of a non-HRTF context: the reference keeps ONE PostProcess variant per device (core/device.h) and so does the
// context.  Stabilizer and Bs2b decode with the B-Format decoder installed under them; HRTF contexts are DeviceLayout::hrtf.
enum class PostKind : uint32_t { None, AmbiDec, Stabilizer, Bs2b, Uhj, Tsme };

// One effect slot: what is attached to it (not owned; each may be null) and where its effects add into.  target: the slot whose
// wet bus that is (oalgpu_slot_set_target: AL_EFFECTSLOT_TARGET_SOFT, alc/alu.cpp:627-632 and :2220-2249), -1: the device's lines;
// depth: what host/slot_order.cpp makes of the graph -- recomputed when a target changes, read by RunEffects (api_slots.hip)
struct EffectSlot {
    oalgpu_convolution *conv{nullptr};     // convolution reverb
    oalgpu_reverb *reverb{nullptr};        // EAX reverb
    oalgpu_effect *effect{nullptr};        // equalizer / modulator / echo / dedicated
    int32_t target{-1};
    uint32_t depth{0};
};

struct BusTransport;
struct oalgpu_context {
    oalgpu_context_desc desc{};
    bool exact{true};
    hipStream_t stream{nullptr};
    bool ownStream{true};
    hipEvent_t evStart{nullptr}, evVoice{nullptr}, evEnd{nullptr};
    // oalgpu_mix_update pipelines two streams when the context owns them: the voice kernel of
    // update k+1 (main stream) overlaps the bus reduction and the post-process of update k
    // (post stream).  The per-workgroup partial buses are double-buffered for that.
    hipStream_t postStream{nullptr};
    // (contexts whose voice launch may span several updates, see pendingMix, cycle through kPartSets sets: two launches in flight)
    static constexpr uint32_t kPartSets = 2u * kSpanMax;
    hipEvent_t evVoiceDone[2]{nullptr, nullptr}, evReduceDone[kPartSets]{}, evPostDone{nullptr};
    uint32_t parity{0};                     // the set of partial buses the next update's sums go into
    uint32_t numSets{2};
    uint32_t voiceLaunches{0};              // evVoiceDone alternates per LAUNCH
    hipEvent_t lastVoiceEvent{nullptr};     // bound to the voice launch submitted last (null: none yet)
    bool postPending{false};
    // A pipelined oalgpu_mix_update is SUBMITTED one library call late: if that next call is oalgpu_param_block_apply, the block's
    // records are installed by the update's own voice kernel -- every wavefront applies the records of the voices it has just
    // mixed, in its epilogue -- and neither ApplyParamsKernel nor its two dispatch gaps stand between two voice kernels.
    // Where the voice kernel has a bounded-run form (Wave16HasSpan) the deferred updates form a short queue: an update whose block
    // has been handed over waits for the next one while the main stream is busy (or while fewer than launchSpan wait), and ONE
    // launch then mixes them all, update by update (RunMixSpan).  Anything that flushes today submits the whole queue.
    struct PendingUpdate { uint32_t samples{0}; int post{0}; oalgpu_param_block *behind{nullptr}; };    // behind: installed after its voices
    struct { uint32_t count{0}; PendingUpdate u[kSpanMax]; bool active() const { return count != 0; } } pendingMix;
    uint64_t spanCounts[kSpanMax]{}, silentPosts{0};   // oalgpu_context_launch_stats
    uint64_t mainStreamGuards{0}, guardQueries{0};     // oalgpu_context_guard_stats
    uint32_t launchSpan{0};                 // oalgpu_context_set_launch_span: 0 automatic, 1 never, 2 .. kSpanMax exactly that many
    // the pipelined host boundary (oalgpu_voice_move_async / oalgpu_read_output_async): pinned ring slots
    static constexpr uint32_t kIoSlots = 4;
    oalgpu_voice_move *panHost[kIoSlots]{};
    size_t panCap{0};
    hipEvent_t panApplied[kIoSlots]{};
    uint32_t panNext{0};
    float *outHost[kIoSlots]{};
    hipEvent_t outDone[kIoSlots]{};
    uint32_t outNext{0};
    size_t outFloats{0};
    // Where the box lets the host store into device memory (large BAR), the move slots ARE device memory: the installing kernel
    // reads its records out of HBM instead of over PCIe (3 us less in front of the voice kernel, tools/ubench_largebar.hip).
    bool panInBar{false};
    // Once oalgpu_read_output_async has been used on an HRTF context, the post-process kernel stores the two output lines into
    // the next ring slot itself and raises the slot's sequence number (pinned, 64 bytes apart) behind them: reading the output
    // back costs the host no runtime call.  outRingWritten: the update submitted last did so, for slot outNext % kIoSlots.
    // oalgpu_voice_events_async: what changed about the voices since the last report, into pinned ring slots
    static constexpr uint32_t kEvCap = 1024;
    uint32_t *evHost[kIoSlots]{};
    hipEvent_t evDone[kIoSlots]{};
    uint32_t evNext{0};
    DevBuf<uint32_t> evSnapshot, evCounters;
    bool outRing{false}, outRingWritten{false};
    bool outViaRing[kIoSlots]{};
    uint32_t outSeq{0}, outSlotSeq[kIoSlots]{};    // every launch that writes a slot raises ITS number
    uint32_t outArrivedTotal{0};                   // what outArrived (the FIR workgroups of every slot-writing launch: it only grows) reads by now
    // What the host already knows to be finished saves it runtime calls: an output that has been waited for proves its update's
    // whole chain done (moves installed, voices mixed, reduced, post-processed), so the checks in front of a slot's or a
    // partial-bus buffer's reuse need not ask the runtime.  Updates are numbered from 1 as they are submitted.
    // oalgpu_mix_update of a pipelined HRTF context without effect slots and without a collective: reduction and post-process
    // are ONE launch (LaunchReducePostFused).  fuseReduce: this update's reduction was held back for it (oalgpu_mix_voices_overlapped
    // -> oalgpu_post_process_overlapped); reducedEpoch: what the launch's counter of reduction workgroups reads when they are through.
    bool fuseReduce{false}, reduceHeld{false};
    // silentPost: the held reduction of this update also does what is left of the post-process of silent dry lines (api.hip:
    // ReduceShiftSilent); dryWriter (sticky): something other than the reduction's zero fill may have written the dry lines
    bool silentPost{false}, dryWriter{false};
    DeviceLayout heldL{};
    uint32_t heldParity{0};
    DevBuf<uint32_t> reducedCount;
    uint32_t reducedEpoch{0};
    hipEvent_t lastPostEvent{nullptr};      // what JoinPost waits for: evPostDone, or the fused launch's own event
    uint64_t updatesSubmitted{0}, updatesKnownDone{0};
    uint64_t reduceUpdate[kPartSets]{}, panUpdate[kIoSlots]{}, outUpdate[kIoSlots]{};
    uint32_t *outFlags{nullptr};
    DevBuf<uint32_t> outArrived;
    float *partHrtfBuf[kPartSets]{};
    float *partLinesBuf[kPartSets]{};
    bool timing{false}, timed{false};
    DeviceLayout L{};
    HrtfStoreDev hrtfDev{};
    HrtfData hrtfHost;
    bool hrtfLoaded{false};
    uint32_t hrtfGeneration{0};            // bumped by every oalgpu_hrtf_load_mhr: parameter blocks carry HRIR indices of ONE store
    bool carryAccum{true};
    bool useWave{false};                   // FAST contexts without sends (HRTF, or <= 8 dry lines): voice_wave.hip
    uint32_t groupsAllocated{0};           // workgroups the partial-bus buffers were sized for (oalgpu_context_create)
    std::vector<EffectSlot> slots;               // per effect slot
    std::vector<uint32_t> slotOrder;             // the order RunEffects goes through them: a permutation, by descending depth
    DevBuf<uint32_t> reverbTicket;               // mix-out order word of a reverb batch launch

    DevBuf<float> tables;
    DevBuf<BufferItem> buffers;
    DevBuf<uint32_t> startDelay;           // [voice] samples until a delayed voice starts
    DevBuf<uint32_t> queueDone;            // [voice] buffers a streaming voice has played through
    // the host's record of every buffer handle (its HBM copy, loop length, who holds it) and of what each voice slot holds:
    // host/buffer_table.hpp has the lifetime rules (oalgpu_buffer_release), api_buffers.hip frees what they hand back
    BufferTable buf;
    DevBuf<VoiceCtl> ctl;
    DevBuf<float> prev, hrtfOld, hrtfTgt, hist, gainCur, gainTgt, sendCur, sendTgt;
    DevBuf<BiquadSlot> dfilt, sfilt;
    DevBuf<float> partLines, partLines2, partHrtf, partHrtf2, partHrtfMore, bus, streams;
    DevBuf<uint32_t> lineGains;
    DevBuf<AmbiScaleState> ambi;
    DevBuf<NfcState> nfc;
    NfcDesign nfcDevice{};                   // DeviceBase::mNFCtrlFilter (after init(w1))
    float nfcAvgDist{0.0f};                  // DeviceBase::AvgSpeakerDist (oalgpu_context_set_nfc_distance; 0: not told)
    DevBuf<NfcRecord> nfcRecDev;             // the source stage's NFC records of a synchronous call (SourceNfcKernel -> ApplyNfcKernel)
    DevBuf<unsigned long long> phaseTimes;  // OALGPU_CTX_PROFILE: the measurement variant's stamps
    WaveProf prof{nullptr, 0u};
    const WaveProf *profArg() const { return prof.times ? &prof : nullptr; }
    DevBuf<AmbiMapEntry> dryMap, wetMaps;   // MixParams::AmbiMap of the dry bus / of every slot's wet bus
    DevBuf<PanRecord> panRecs;
    std::vector<VoiceCtl> ctlHost;          // oalgpu_voices_readback: staging
    std::vector<uint32_t> doneHost;
    DevBuf<TargetRecord> tgtRecs;           // oalgpu_voice_set_hrtf_targets: staging
    DevBuf<float> tgtCoeffs;
    bool serialOnly{false};                // OALGPU_CTX_SERIAL: no two-stream pipeline
    // multi-GPU (oalgpu_comm_init / oalgpu_comm_init_host): how this rank's bus block gets summed into rank 0's,
    // right behind the partial-bus reduction, on the stream that runs it
    struct BusTransport *comm{nullptr};
    int commRank{0}, commWorld{1};
    // several contexts on one device (oalgpu_context_attach: ProcessContexts, alc/alu.cpp:2177-2273).  The device context
    // updates its attached contexts -- their voices before its own voice kernel, their effect slots before the merge -- and ONE
    // launch (BusMergeKernel) adds their dry + real lines into its own behind its reduction.
    oalgpu_context *attachedTo{nullptr};   // (attached context) the device context that updates it
    std::vector<int32_t> attachMap;        // (attached context) its line i -> line of the device context's dry + real block, or -1
    hipEvent_t evBusFinal{nullptr};        // (attached context) behind its last launch of an update: its reduction or its last effect kernel
    std::vector<oalgpu_context*> attached; // (device context) in attach order
    DevBuf<BusMergeHead> mergeHeads;       // (device context) the merge's table, rebuilt by attach / detach: a head per
    DevBuf<BusMergeRow> mergeRows;         // destination line that has contributors, a row per contributing line
    uint32_t mergeLines{0};
    hipEvent_t evMerged{nullptr};          // (device context) behind the merge: the attached contexts' next reductions wait for it
    bool mergeInFlight{false};             // a merge was launched since the host last waited for the device context
    // the stage behind the buses (api_poststage.hip): the one post-process of a non-HRTF context and what each kind keeps
    PostKind post{PostKind::None};
    // the B-Format decoder (oalgpu_set_bformat_decoder: AmbiDec, and under Stabilizer and Bs2b)
    bool decDual{false};
    uint32_t decOut{0};
    DevBuf<float> decGainsHf, decGainsLf, decBands;
    DevBuf<SplitterState> decSplit;
    // the output format (oalgpu_set_output; oalgpu_read_output: dither, PCM)
    int outType{6};                        // DevFmtType order: 0 i8, 1 u8, 2 i16, 3 u16, 4 i32, 5 u32, 6 f32
    float ditherDepth{0.0f};
    uint32_t ditherSeed{22222};
    // the output limiter (oalgpu_set_output_limiter; RunLimiter behind every post-process, HRTF included): its constants and device state
    bool limOn{false};
    LimiterConsts lim{};
    DevBuf<float> limState;
    // the stereo encoder (oalgpu_set_uhj_encoder: Uhj, 3 dry / 2 real lines; oalgpu_set_tsme_encoder: Tsme, 4 dry / 2 real
    // lines): its quality, FIR taps and device state
    int encQuality{-1};
    DevBuf<float> encTaps, encState;
    // the front stabilizer (oalgpu_set_front_stabilizer: Stabilizer): the real lines of FrontLeft / FrontRight / FrontCenter,
    // its constants and device state
    uint32_t stabLeft{0}, stabRight{0}, stabCenter{0};
    StabilizerConsts stab{};
    DevBuf<float> stabState;
    // the bs2b crossfeed (oalgpu_set_crossfeed: Bs2b): the real lines of FrontLeft / FrontRight, its constants and device state
    uint32_t cfLeft{0}, cfRight{0};
    CrossfeedConsts cf{};
    DevBuf<float> cfState;
    // speaker distance compensation (oalgpu_set_distance_comp; behind the limiter of non-HRTF contexts): per
    // output line its delay and gain, and the delay lines
    uint32_t distLines{0};
    DevBuf<uint32_t> distDelays;
    DevBuf<float> distGains, distHist;
    DevBuf<unsigned char> pcm;
    // HRTF store
    DevBuf<float> hFieldDist, hCoeffs;
    DevBuf<uint8_t> hEvCount, hDelays;
    DevBuf<uint16_t> hAzCount, hIrOffset;
    // DirectHrtfState
    DevBuf<SplitterState> dSplit, dSplit2;  // the post-process's splitter states; the fused FAST post-process reads one and files the other
    uint32_t dSplitCur{0};                  // which of the two holds the current states
    DevBuf<float> carryBuf;                 // HrtfAccumData as the fused post-process leaves it (1152 x 2): the next reduction's carry
    float dSplitCoeff{0.0f};                // the splitters' coefficient (one crossover for all channels) ...
    float runPower[4]{1.0f, 0.0f, 1.0f, 1.0f};  // ... and their transition over a run of runPowerSeg samples (SplitterRunPowers)
    uint32_t runPowerSeg{0};
    DevBuf<uint32_t> postArrived;           // the fused post-process's channel counter (only ever grows) ...
    uint32_t postEpoch{0};                  // ... and the value it has reached after the last launch
    const ParamRecord *nextRecs{nullptr};   // the block the voice kernel being launched installs in its epilogue (RunMixUpdate)
    const int32_t *nextMap{nullptr};
    const float *nextRows{nullptr};
    bool carryInBuf{false};                 // the carried accumulator is in carryBuf (else: in the bus block's accumulator region)
    DevBuf<float> dHfScale, dCoeffs, dTemp;
    uint32_t dIrSize{0};
    bool directSet{false};
    // staging
    DevBuf<ParamRecord> paramDev;
    std::vector<ParamRecord> paramHost;
    DevBuf<VoiceInitRecord> initDev;
    std::vector<VoiceInitRecord> initPending;
    // 3D source parameters on the GPU (api_sources.hip): ContextParams and alu.cpp's scales, what CalcAttnVoiceParams reads of
    // every effect slot (host copy and device copy), the resampler tables' constants (uploaded with the first use), each voice
    // slot's Voice::mFrequency (0: not started through oalgpu_voice_init), and the source records' staging
    oalgpu_listener_params listener{{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f}, {}, {},
        1.0f, 1.0f, 0.99426f, 1.0f, 343.3f, 0, OALGPU_DISTANCE_DISABLE, 1.0f, 1.0f, {1.0f, 1.0f, 1.0f}};
    std::vector<oalgpu_slot_environment> slotEnvHost;
    DevBuf<oalgpu_slot_environment> slotEnv;
    DevBuf<ResamplerConsts> rsConsts;
    std::vector<uint32_t> voiceFreq;
    DevBuf<SourceRecord> srcDev;
    std::vector<SourceRecord> srcHost;
    std::vector<uint32_t> srcVoices;        // (the voices of srcHost: a voice named twice keeps its last record)
    DevBuf<ChannelSourceRecord> chanDev;    // channel sources (oalgpu_voice_set_channel_sources): their staging; srcVoices: the
    std::vector<ChannelSourceRecord> chanHost;      // channel voices in the order of their records
    // ambisonic sources (oalgpu_voice_set_ambi_sources): DeviceBase::mAmbiOrder / m2DMixing (0: not told), the upsamplers the
    // context was given ([(source order - 1) * 2 + is_2d], kAmbiMatrix floats each, host and device), RotatorCoeffArray on the
    // device, the records' staging
    uint32_t ambiOrder{0};
    bool ambiMix2d{false};
    bool ambiUpGiven[8]{};
    std::vector<float> ambiUpHost;
    DevBuf<float> ambiUpDev, ambiRotDev;
    DevBuf<AmbiSourceRecord> ambiDev;
    std::vector<AmbiSourceRecord> ambiHost;
    // callback sources (oalgpu_voice_init_callback): the host's mirror of what Voice::mix keeps for them
    struct CbVoice {
        uint32_t voice{0}; int32_t buffer{-1}; uint32_t frameBytes{4}, capacityFrames{0};
        oalgpu_callback_fn fn{nullptr}; void *user{nullptr};
        std::vector<char> data;                    // BufferStorage::mData of the callback buffer: numBlocks blocks valid
        uint32_t numBlocks{0}, blockOffset{0};     // Voice::mNumCallbackBlocks / mCallbackBlockOffset (samples per block = 1)
        bool stopped{false};                       // VoiceFlag::CallbackStopped
        int32_t position{0}; uint32_t frac{0}, step{0};        // mPosition / mPositionFrac / mStep
        int state{OALGPU_VOICE_PLAYING}; bool hasBuffer{true}; // mPlayState / mCurrentBuffer != nullptr
        char *pinned[2]{nullptr, nullptr}; hipEvent_t copied[2]{nullptr, nullptr}; uint32_t slot{0};
        size_t allocBytes{0};                      // of the device buffer and each pinned one
        bool retired{false};                       // its voice slot became another source: the entry may be reused
    };
    std::vector<CbVoice> cbVoices;
    std::vector<int32_t> cbOfVoice;                // [voice] index into cbVoices, -1 = not a callback source

    // ---- the resident voice kernel (OALGPU_CTX_RESIDENT; protocol and device side: kernels.hpp ResidentDoor, voice_wave.hip) ----
    // One launch of the HRTF voice kernel stays on the machine while the host only calls oalgpu_param_block_apply,
    // oalgpu_mix_update, oalgpu_read_output_async and oalgpu_output_wait.  Per update the host writes a doorbell slot and
    // launches the update's reduction (reduce stream) and post-process (post stream), which wait for device counters.  Any
    // other entry point parks the kernel first (UseDevice): it finishes what has been rung and ends, and whatever the entry
    // point puts on the main stream runs behind it in stream order.
    struct ResidentState {
        bool enabled{false};                       // the context was created with OALGPU_CTX_RESIDENT and its layout has a resident kernel
        bool ready{false}, failed{false};          // buffers and streams exist; the mode gave up (the context then launches per update)
        bool running{false};                       // a launch is on the main stream that has not been told to leave
        hipStream_t reduceStream{nullptr};
        ResidentDoor *door{nullptr};               // the host's view (the device reads the same address)
        bool doorInBar{false};
        DevBuf<uint32_t> counters;                 // [kRcCount][16]
        uint32_t *hostFlags{nullptr};              // pinned [kRhCount][16]
        DevBuf<float> part;                        // kResidentSets sets of partial buses
        size_t setFloats{0};
        uint32_t next{0};                          // the next update's index (counts this context's resident updates)
        uint32_t endSeq{0};                        // where the running launch ends by itself
        uint32_t launches{0}, startedTotal{0};
        uint32_t launchBase{0};                    // the running launch's first update
        // A launch pays for itself over a few dozen updates (its first updates run at the launched path's pace, and the block
        // ends with the pipeline's drain: 45.5 against 44.5 us per update for blocks of 20, 38.8 against 42.9 for blocks of 50,
        // tools/resident_block_cost.py).  A host that keeps it short -- a synchronisation every 20 updates, parameters set the
        // launched way before every update -- is better off with a launch per update: after three launches in a row that covered
        // fewer than 32 updates the context launches per update for a while, then tries again.
        uint32_t shortRuns{0}, cooldown{0};
        uint32_t shortRun{32};                     // launches that cover fewer updates count as short (0: never fall back)
        uint32_t awaitStarted{0};                  // the launch id whose "every workgroup has started" word the host has yet to see
        uint32_t maxUpdates{4096};
        uint32_t setUses[kResidentSets]{};         // updates that went into each partial set so far
        uint32_t posts{0};                         // post-processes launched in this mode
        uint32_t firGroups{0}, redGroups{0}, groupsPerCu{0};
        oalgpu_param_block *pendingBlock{nullptr}; // oalgpu_param_block_apply: rides in the next update's doorbell slot
        hipEvent_t copyPending{nullptr};           // a copy out of the bus block queued on the post stream: the next reduction waits for it
        // the launches' own times (events bound to the dispatch), collected when the launch is known to have ended
        static constexpr uint32_t kEv = 4;
        hipEvent_t evStart[kEv]{}, evStop[kEv]{};
        uint32_t evFirst[kEv]{}, evLast[kEv]{};    // the updates the launch of that event pair covered: [first, last)
        bool evOpen[kEv]{};
        bool timeLaunches{false};                  // oalgpu_set_timing: the launches carry their events
        double kernelMs{0.0};
        uint64_t kernelUpdates{0}, kernelLaunches{0}, parks{0};
    } res;

    ~oalgpu_context()
    {
        for(int h = 0; buf.inRange(h); ++h) (void)hipFree(buf.at(h).storage);    // (what the table still holds)
        for(uint32_t k = 0; k < kIoSlots; ++k)
        {
            if(panHost[k]) (void)(panInBar ? hipFree(panHost[k]) : hipHostFree(panHost[k]));
            if(outHost[k]) (void)hipHostFree(outHost[k]);
            if(evHost[k]) (void)hipHostFree(evHost[k]);
            if(evDone[k]) (void)hipEventDestroy(evDone[k]);
            for(hipEvent_t e : {panApplied[k], outDone[k]}) if(e) (void)hipEventDestroy(e);
        }
        if(outFlags) (void)hipHostFree(outFlags);
        if(res.door) (void)(res.doorInBar ? hipFree(res.door) : hipHostFree(res.door));
        if(res.hostFlags) (void)hipHostFree(res.hostFlags);
        for(uint32_t k = 0; k < ResidentState::kEv; ++k)
            for(hipEvent_t e : {res.evStart[k], res.evStop[k]}) if(e) (void)hipEventDestroy(e);
        if(res.reduceStream) (void)hipStreamDestroy(res.reduceStream);
        for(hipEvent_t e : {evBusFinal, evMerged}) if(e) (void)hipEventDestroy(e);
        if(evStart) (void)hipEventDestroy(evStart);
        if(evVoice) (void)hipEventDestroy(evVoice);
        if(evEnd) (void)hipEventDestroy(evEnd);
        for(hipEvent_t e : {evVoiceDone[0], evVoiceDone[1], evPostDone})
            if(e) (void)hipEventDestroy(e);
        for(hipEvent_t e : evReduceDone) if(e) (void)hipEventDestroy(e);
        if(postStream) (void)hipStreamDestroy(postStream);
        if(stream && ownStream) (void)hipStreamDestroy(stream);
    }
};

struct oalgpu_param_block {
    DevBuf<ParamRecord> recs;
    uint32_t count{0};
    int device{0};
    uint32_t hrtfGeneration{0};                             // of the store the records' HRIR indices and weights were taken from
    DevBuf<int32_t> voiceToRec;                             // [voice of the context] -> index of its record in the block, or -1: how a
                                                            // voice kernel's wavefront finds the records of the voices it mixed
    uint32_t mapVoices{0};
    DevBuf<float> rows;                                     // [record][irStride][2]: the records' blended target HRIRs (resident contexts)
    DevBuf<NfcRecord> nfc;                                  // [record]: the records' NfcFilter adjusts (blocks made from sources on a
                                                            // near-field context; null otherwise), installed with the records
    std::vector<std::pair<uint32_t, uint32_t>> cbSteps;     // (voice, mStep) of the callback voices in the block
    oalgpu_context *heldBy{nullptr};                        // a resident context that keeps the block for its next update (res.pendingBlock)
    oalgpu_context *queuedBy{nullptr};                      // a context whose deferred updates wait with the block between them (pendingMix)
};

// The one exchange of a sharded update: the bus block [dry + real lines | wet buses |
// HrtfAccumData] of every rank is summed into rank 0's, in place, on the stream that just produced it.  Two
// transports behind one interface: RCCL (ncclReduce over xGMI, one process per GPU) and a host-staged one
// (every rank's block through pinned memory into a shared-memory ring, summed by rank 0's stream in rank order)
// for ranks that RCCL cannot serve -- several processes on ONE GPU, which is how the N > 1 code of this library
// is exercised on a one-GPU box (tests/test_multi_rank.py).
struct BusTransport {
    virtual ~BusTransport() = default;
    virtual int reduceToRoot(oalgpu_context *c, hipStream_t s) = 0;
    virtual int ranks() const = 0;              // ranks the transport itself counts (RCCL: ncclCommCount)
    virtual const char *kind() const = 0;
};

namespace oalgpu { extern thread_local std::string gLastError; }

// ---- shared between the translation units (definitions: api.hip unless noted) ----
int FlushPendingMix(oalgpu_context *c);
int DeferBlockBehindPending(oalgpu_context *c, struct oalgpu_param_block *b);   // oalgpu_param_block_apply on a context with deferred updates
int UseCtx(oalgpu_context *c);
// the update's pieces that other units launch: a context's voices and reduction on its main stream (oalgpu_mix_voices; what a
// device context does for each attached context), the carried accumulator a reduction adds, the one-launch HRTF post-process
int MixVoicesSerial(oalgpu_context *c, uint32_t samples_to_do);
const float *CarrySource(oalgpu_context *c, bool carry);
int PostDirectHrtfFused(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do, hipEvent_t evDone, bool resident = false);
int RebalanceWaveGroups(oalgpu_context *c);                        // (the voice kernel's grid, after a reverb came or went)
// the resident voice kernel's host side (api_resident.hip)
namespace oalgpu { void ParkResidentContexts(int device); }
bool ResidentWanted(const oalgpu_context *c, int post_process);
int FlushResidentBlock(oalgpu_context *c);
int ResidentSubmit(oalgpu_context *c, uint32_t samples_to_do);     // 1: the update goes the launched way after all
void ResidentCollectTimes(oalgpu_context *c, bool all);
int ResidentCheckError(oalgpu_context *c);
// several contexts on one device (api_attach.hip)
int RefuseAttached(const oalgpu_context *c, const char *who);
int MixAttached(oalgpu_context *c, uint32_t samples_to_do);
int MergeAttached(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do);
void DetachForDestroy(oalgpu_context *ctx);
// the effect slots (api_slots.hip)
int RunEffects(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do);
uint32_t AttachedReverbs(const oalgpu_context *c);
int UseCtxResident(oalgpu_context *c);
void RetireCallbackVoice(oalgpu_context *c, uint32_t voice);
void NoteCallbackSteps(oalgpu_context *c, const uint32_t *voices, const oalgpu_voice_params *params, size_t count);
int FlushInits(oalgpu_context *c);
int AllocStreamRows(oalgpu_context *c);
uint32_t DeviceComputeUnits(int device);
int JoinPost(oalgpu_context *c);
// what every setter that may follow a deferred update starts with: the update is submitted, a parameter block that waits for a
// resident update goes in (it was applied BEFORE this call, as on the launched path), and a null context is `who`'s error
int BeginSetter(oalgpu_context *c, const char *who);
int RunSpeakerPost(oalgpu_context *c, hipStream_t s, uint32_t samplesToDo);   // api_poststage.hip (a non-HRTF update's whole post stage)
int RunLimiter(oalgpu_context *c, hipStream_t s, uint32_t samplesToDo);       // api_poststage.hip (behind an HRTF post-process)
bool RingEligible(const oalgpu_context *c);                        // api_output.hip
// RealOut: the real output lines, or the dry lines themselves where the device has none (core/device.h:300)
inline float *RealOut(const oalgpu_context *c) { return c->L.numReal ? c->L.bus + size_t{c->L.numDry} * kLine : c->L.bus; }
inline uint32_t RealOutLines(const oalgpu_context *c) { return c->L.numReal ? c->L.numReal : c->L.numDry; }
bool HostStoresReachDevice(oalgpu_context *c);                     // api_voices.hip
// buffer handles (api_buffers.hip): the tail of every registration -> the handle, or an error; the storage a drop handed back
int RegisterBuffer(oalgpu_context *c, void *storage, BufferItem item, uint32_t loopLen, int parent);
void FreeStorage(const std::vector<void*> &freed);
// voices (api_voices.hip).  What an entry point that looks at the voices starts with, like BeginSetter: `argsOk` false is
// `who`'s error; then UseCtx, the deferred starts (FlushInits) and, with `sync`, oalgpu_sync.  PendStart: a deferred start.
inline bool VoiceOk(const oalgpu_context *c, uint32_t voice) { return c && voice < c->L.numVoices; }
int BeginVoiceCall(oalgpu_context *c, bool argsOk = true, const char *who = "", bool sync = false);
void PendStart(oalgpu_context *c, const VoiceInitRecord &rec);
// a parameter block whose records are in place: its voice -> record map and, where the voice kernel installs blocks, its rows
int FinishParamBlock(oalgpu_context *c, struct oalgpu_param_block *b, const uint32_t *voices, size_t count);
oalgpu::HrtfStoreDev HostStoreView(const oalgpu::HrtfData &h);     // api_hrtf.hip
// a near-field context's side of the source stage (api_sources.hip): what SourceNfcKernel reads of the context, and the install
// of `count` NFC records behind the parameter records they belong to
oalgpu::NfcSetup NfcSetupOf(const oalgpu_context *c);
void ApplyNfcRecords(oalgpu_context *c, const oalgpu::NfcRecord *recs, uint32_t count);
int ServiceCallbacks(oalgpu_context *c, uint32_t samplesToDo);     // api_callback.hip
int CommReduceBus(oalgpu_context *c, hipStream_t s);               // api_comm.hip

