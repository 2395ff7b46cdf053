// Several contexts on one device (oalgpu_context_attach: ProcessContexts, alc/alu.cpp:2177-2273; include/oalgpu.h):
// the links, the merge's table, and what a device context's update does for its attached contexts.
// (Part of the C-ABI shim: see api.hip.)
#include "api_context.hpp"

int RefuseAttached(const oalgpu_context *c, const char *who)
{
    if(!c->attachedTo) return OALGPU_OK;
    return Fail(OALGPU_ERR_INVALID, std::string(who) + ": the context is attached (oalgpu_context_attach): its device context updates it");
}

// (device context) the attached contexts' voices and reductions of this update, each on its own main stream, in front of the
// device context's own voice kernel: the kernels run side by side
int MixAttached(oalgpu_context *c, uint32_t samples_to_do)
{
    for(oalgpu_context *a : c->attached) { if(int rc = MixVoicesSerial(a, samples_to_do)) return rc; }
    return OALGPU_OK;
}

// (device context) behind its own reduction on stream `s`, in front of its effect slots and post stage: the attached contexts'
// effect slots, then their lines into the device context's (BusMergeKernel) once their last launches are through
int MergeAttached(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do)
{
    for(oalgpu_context *a : c->attached)
    {
        if(int rc = RunEffects(a, a->stream, samples_to_do)) return rc;
        HIP_TRY(hipEventRecord(a->evBusFinal, a->stream));
        HIP_TRY(hipStreamWaitEvent(s, a->evBusFinal, 0));
    }
    LaunchBusMerge(s, c->mergeHeads.p, c->mergeRows.p, c->mergeLines, samples_to_do);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->evMerged, s));
    c->mergeInFlight = true;
    return OALGPU_OK;
}

// The merge's table of a device context, from its attached contexts' maps: per destination line the contributing lines in
// attach order (within a context: in line order).  The caller has waited for everything that may still read the old table.
static int RebuildMergeTable(oalgpu_context *d)
{
    const uint32_t lines = d->L.numDry + d->L.numReal;
    std::vector<BusMergeHead> heads;
    std::vector<BusMergeRow> rows;
    std::vector<int32_t> last(lines, -1);
    for(uint32_t line = 0; line < lines; ++line)
        for(const oalgpu_context *a : d->attached)
            for(size_t i = 0; i < a->attachMap.size(); ++i)
            {
                if(a->attachMap[i] != int32_t(line)) continue;
                const int32_t r = int32_t(rows.size());
                rows.push_back(BusMergeRow{a->L.bus + i * kLine, -1, 0u});
                if(last[line] < 0) heads.push_back(BusMergeHead{d->L.bus + size_t{line} * kLine, r, 0u});
                else rows[size_t(last[line])].next = r;
                last[line] = r;
            }
    // (built beside the old table and swapped in whole: a failed allocation leaves the old one, and its contexts merged)
    DevBuf<BusMergeHead> newHeads;
    DevBuf<BusMergeRow> newRows;
    if(!heads.empty())
    {
        HIP_TRY(newHeads.alloc(heads.size())); HIP_TRY(newHeads.upload(heads.data(), heads.size()));
        HIP_TRY(newRows.alloc(rows.size())); HIP_TRY(newRows.upload(rows.data(), rows.size()));
    }
    std::swap(d->mergeHeads.p, newHeads.p); std::swap(d->mergeHeads.n, newHeads.n);
    std::swap(d->mergeRows.p, newRows.p); std::swap(d->mergeRows.n, newRows.n);
    d->mergeLines = uint32_t(heads.size());
    return OALGPU_OK;
}

static void Unlink(oalgpu_context *a)
{
    oalgpu_context *d = a->attachedTo;
    d->attached.erase(std::remove(d->attached.begin(), d->attached.end(), a), d->attached.end());
    a->attachedTo = nullptr;
    a->attachMap.clear();
    d->mergeInFlight = false;
}

int oalgpu_context_attach(oalgpu_context *d, oalgpu_context *a, const int32_t *line_map)
{
    const std::string w = "oalgpu_context_attach: ";
    if(!d || !a || !line_map) return Fail(OALGPU_ERR_INVALID, w + "null argument");
    if(d == a) return Fail(OALGPU_ERR_INVALID, w + "a context cannot be attached to itself");
    if(a->attachedTo) return Fail(OALGPU_ERR_INVALID, w + "the context is already attached");
    if(d->attachedTo) return Fail(OALGPU_ERR_INVALID, w + "the device context is itself attached (no nesting)");
    if(!a->attached.empty()) return Fail(OALGPU_ERR_INVALID, w + "the context has attached contexts of its own (no nesting)");
    if(d->desc.device != a->desc.device) return Fail(OALGPU_ERR_INVALID, w + "the contexts are on different devices");
    if(d->desc.sample_rate != a->desc.sample_rate) return Fail(OALGPU_ERR_INVALID, w + "the contexts have different sample rates");
    if(a->L.hrtf) return Fail(OALGPU_ERR_INVALID, w + "an HRTF context cannot be attached (HRTF voices belong to the device context)");
    if(a->post != PostKind::None) return Fail(OALGPU_ERR_INVALID, w + "the context has a post-process installed (the device context post-processes)");
    if(a->limOn) return Fail(OALGPU_ERR_INVALID, w + "the context has an output limiter (the device context limits)");
    if(a->distLines) return Fail(OALGPU_ERR_INVALID, w + "the context has distance compensation (the device context compensates)");
    if(a->outType != OALGPU_OUT_F32 || a->ditherDepth > 0.0f)
        return Fail(OALGPU_ERR_INVALID, w + "the context has an output conversion (oalgpu_set_output: the device context converts)");
    if(d->comm || a->comm) return Fail(OALGPU_ERR_INVALID, w + "a context with a collective (oalgpu_comm_init) takes and is no attachment");
    if(!a->ownStream) return Fail(OALGPU_ERR_INVALID, w + "the context is on a caller-owned stream (oalgpu_set_stream)");
    const uint32_t srcLines = a->L.numDry + a->L.numReal, dstLines = d->L.numDry + d->L.numReal;
    for(uint32_t i = 0; i < srcLines; ++i)
        if(line_map[i] < -1 || line_map[i] >= int32_t(dstLines))
            return Fail(OALGPU_ERR_INVALID, w + "map entry " + std::to_string(i) + " is out of range (-1 .. " + std::to_string(dstLines - 1u) + ")");
    // the work in flight of both (a resident voice kernel leaves, a deferred update is submitted)
    if(int rc = oalgpu_sync(d)) return rc;
    if(int rc = oalgpu_sync(a)) return rc;
    // ordering between streams of one device only: no system-scope fence (see oalgpu_context_create)
    if(!a->evBusFinal) HIP_TRY(hipEventCreateWithFlags(&a->evBusFinal, hipEventDisableTiming | hipEventDisableSystemFence));
    if(!d->evMerged) HIP_TRY(hipEventCreateWithFlags(&d->evMerged, hipEventDisableTiming | hipEventDisableSystemFence));
    a->attachMap.assign(line_map, line_map + srcLines);
    a->attachedTo = d;
    d->attached.push_back(a);
    d->dryWriter = true;                    // (sticky: the merge writes the device context's dry lines)
    if(int rc = RebuildMergeTable(d))
    {
        Unlink(a);
        (void)RebuildMergeTable(d);
        return rc;
    }
    return OALGPU_OK;
}

int oalgpu_context_detach(oalgpu_context *a)
{
    if(!a) return Fail(OALGPU_ERR_INVALID, "oalgpu_context_detach: null argument");
    oalgpu_context *d = a->attachedTo;
    if(!d) return Fail(OALGPU_ERR_INVALID, "oalgpu_context_detach: the context is not attached");
    if(int rc = oalgpu_sync(d)) return rc;          // (waits for the attached contexts' streams as well)
    Unlink(a);
    return RebuildMergeTable(d);
}

// oalgpu_context_destroy of a context that has, or is, an attachment: the links go whatever the device says
void DetachForDestroy(oalgpu_context *ctx)
{
    if(oalgpu_context *d = ctx->attachedTo)
    {
        (void)oalgpu_sync(d);
        Unlink(ctx);
        (void)RebuildMergeTable(d);
    }
    if(!ctx->attached.empty())
    {
        (void)oalgpu_sync(ctx);
        while(!ctx->attached.empty()) Unlink(ctx->attached.back());
        ctx->mergeLines = 0;
    }
}
