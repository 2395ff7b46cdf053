// Buffer handles: registration, channel views, queue links, release.  Who holds whom and when a handle dies is host/buffer_table.cpp's;
// this file owns the HBM copies and the device's BufferItem rows.
#include "api_context.hpp"

void FreeStorage(const std::vector<void*> &freed)
{
    // (the caller has made sure nothing on the device still reads the storage: hipFree waits for the device besides)
    for(void *p : freed) (void)hipFree(p);
}

/* What every registering entry point ends in.  `storage` is the handle's from here on (null: a view, which holds `parent`
 * instead), `item` its row of the device's table.  A failure gives the handle back, its storage with it. */
int RegisterBuffer(oalgpu_context *c, void *storage, BufferItem item, uint32_t loopLen, int parent)
{
    const int h = c->buf.alloc(storage, loopLen, parent);
    if(h < 0) { (void)hipFree(storage); return Fail(OALGPU_ERR_CAPACITY, "buffer table full"); }
    item.next = 0;
    const hipError_t e = hipMemcpy(c->buffers.p + h, &item, sizeof(item), hipMemcpyHostToDevice);
    if(e == hipSuccess) return h;
    FreeStorage(c->buf.release(h));
    return Fail(OALGPU_ERR_HIP, hipGetErrorString(e));
}

// the start of a registration: its arguments (`refusal` if they are bad), a place in the table, the device
static int BeginRegister(oalgpu_context *c, bool argsOk, const char *refusal)
{
    if(!argsOk) return Fail(OALGPU_ERR_INVALID, refusal);
    if(c->buf.full()) return Fail(OALGPU_ERR_CAPACITY, "buffer table full");
    return UseCtx(c);
}
// loop points of a buffer of sample_len frames: none (0, 0), or start < end <= sample_len
static bool LoopPointsOk(uint32_t sample_len, uint32_t loop_start, uint32_t loop_end)
{ return loop_end <= sample_len && loop_start < (loop_end ? loop_end : 1u); }

int oalgpu_buffer_release(oalgpu_context *c, int buffer)
{
    if(!c || !c->buf.live(buffer)) return Fail(OALGPU_ERR_INVALID, "oalgpu_buffer_release: not a registered buffer");
    if(c->buf.at(buffer).released) return Fail(OALGPU_ERR_INVALID, "oalgpu_buffer_release: released before");
    if(int rc = UseCtx(c)) return rc;
    for(const auto &cb : c->cbVoices)
        if(cb.buffer == buffer && !cb.retired) return Fail(OALGPU_ERR_INVALID, "oalgpu_buffer_release: a callback source's storage is the library's own");
    // initialisations that wait for the next update name their buffers: they are on the device before anything is freed
    if(int rc = FlushInits(c)) return rc;
    FreeStorage(c->buf.release(buffer));
    return OALGPU_OK;
}

int oalgpu_buffer_info(oalgpu_context *c, int buffer, int32_t *live, int32_t *release_pending, uint32_t *references)
{
    if(!c || !c->buf.inRange(buffer)) return Fail(OALGPU_ERR_INVALID, "oalgpu_buffer_info: bad handle");
    const BufferRecord &b = c->buf.at(buffer);
    if(live) *live = b.live ? 1 : 0;
    if(release_pending) *release_pending = (b.live && b.released) ? 1 : 0;
    if(references) *references = b.refs;
    return OALGPU_OK;
}

int oalgpu_buffer_register(oalgpu_context *c, const void *data, int fmt_type, uint32_t frame_step,
    uint32_t sample_len, uint32_t loop_start, uint32_t loop_end)
{
    if(int rc = BeginRegister(c, c && data && fmt_type >= 0 && fmt_type <= OALGPU_FMT_ALAW && frame_step != 0 && sample_len != 0
        && LoopPointsOk(sample_len, loop_start, loop_end), "oalgpu_buffer_register: bad arguments")) return rc;
    const size_t nbytes = size_t{sample_len} * frame_step * kSourceBytesPer[fmt_type];
    void *dev = nullptr;
    HIP_TRY(hipMalloc(&dev, nbytes + 16));
    const hipError_t e = hipMemcpy(dev, data, nbytes, hipMemcpyHostToDevice);
    if(e != hipSuccess) { (void)hipFree(dev); return Fail(OALGPU_ERR_HIP, hipGetErrorString(e)); }
    return RegisterBuffer(c, dev, BufferItem{dev, fmt_type, frame_step, sample_len, loop_start, loop_end, 0},
        loop_end - loop_start, -1);
}

/* IMA4 / MS ADPCM data (FmtIMA4 / FmtMSADPCM, core/buffer_storage.h; LoadSamples, core/voice.cpp:288-484):
 * decoded once, on the GPU, into interleaved 16-bit PCM; the handle then behaves like an OALGPU_FMT_SHORT
 * buffer with frame_step = channels (oalgpu_buffer_channel_view splits a stereo one). */
int oalgpu_buffer_register_adpcm(oalgpu_context *c, const void *data, int adpcm_type, uint32_t channels,
    uint32_t samples_per_block, uint32_t sample_len, uint32_t loop_start, uint32_t loop_end)
{
    if(int rc = BeginRegister(c, c && data && (adpcm_type == OALGPU_ADPCM_IMA4 || adpcm_type == OALGPU_ADPCM_MS) && channels >= 1
        && channels <= 2 && sample_len != 0 && LoopPointsOk(sample_len, loop_start, loop_end)
        && samples_per_block >= (adpcm_type == OALGPU_ADPCM_MS ? 3u : 2u) && samples_per_block <= 65536u,
        "oalgpu_buffer_register_adpcm: bad arguments")) return rc;
    const uint32_t numBlocks = (sample_len + samples_per_block - 1u) / samples_per_block;
    const size_t blockBytes = adpcm_type == OALGPU_ADPCM_MS ? size_t{(samples_per_block - 2u) / 2u + 7u} * channels
        : size_t{(samples_per_block - 1u) / 2u + 4u} * channels;
    const size_t nbytes = size_t{numBlocks} * blockBytes;
    void *comp = nullptr, *pcm = nullptr;
    HIP_TRY(hipMalloc(&comp, nbytes + 16));
    hipError_t e = hipMemcpy(comp, data, nbytes, hipMemcpyHostToDevice);
    if(e == hipSuccess) e = hipMalloc(&pcm, size_t{sample_len} * channels * sizeof(int16_t) + 16);
    if(e != hipSuccess) { (void)hipFree(comp); return Fail(OALGPU_ERR_HIP, hipGetErrorString(e)); }
    LaunchDecodeAdpcm(c->stream, adpcm_type == OALGPU_ADPCM_MS, static_cast<const uint8_t*>(comp), static_cast<int16_t*>(pcm),
        numBlocks, samples_per_block, channels, sample_len);
    e = hipGetLastError();
    if(e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(comp);
    if(e != hipSuccess) { (void)hipFree(pcm); return Fail(OALGPU_ERR_HIP, hipGetErrorString(e)); }
    return RegisterBuffer(c, pcm, BufferItem{pcm, OALGPU_FMT_SHORT, channels, sample_len, loop_start, loop_end, 0},
        loop_end - loop_start, -1);
}

int oalgpu_buffer_channel_view(oalgpu_context *c, int buffer, uint32_t channel)
{
    if(int rc = BeginRegister(c, c && c->buf.usable(buffer), "oalgpu_buffer_channel_view: bad buffer")) return rc;
    BufferItem item{};
    HIP_TRY(hipMemcpy(&item, c->buffers.p + buffer, sizeof(item), hipMemcpyDeviceToHost));
    if(channel >= item.frameStep) return Fail(OALGPU_ERR_INVALID, "oalgpu_buffer_channel_view: channel >= frame_step");
    item.data = static_cast<const char*>(item.data) + size_t{channel} * kSourceBytesPer[item.fmt];
    // (the storage belongs to `buffer`: the view holds it)
    return RegisterBuffer(c, nullptr, item, c->buf.at(buffer).loopLen, buffer);
}

/* streaming sources: a queue of buffers (VoiceBufferItem::mNext, core/voice.h:85).  This is alSourceQueueBuffers' linking
 * (next < 0 ends the queue); oalgpu_voice_init_queue starts a voice on a queue's first buffer (StartVoice, api_voices.hip). */
int oalgpu_buffer_queue_link(oalgpu_context *c, int buffer, int next_buffer)
{
    if(!c || !c->buf.live(buffer) || (next_buffer >= 0 && !c->buf.usable(next_buffer)))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_buffer_queue_link: bad buffer");
    if(int rc = UseCtx(c)) return rc;
    if(int rc = oalgpu_sync(c)) return rc;
    FreeStorage(c->buf.link(buffer, next_buffer));          // the link holds its target
    const int32_t next = next_buffer < 0 ? 0 : next_buffer + 1;
    HIP_TRY(hipMemcpy(reinterpret_cast<char*>(c->buffers.p + buffer) + offsetof(BufferItem, next), &next, sizeof(next),
        hipMemcpyHostToDevice));
    return OALGPU_OK;
}
