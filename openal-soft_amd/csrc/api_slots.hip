// The effect slots of a context (EffectSlot, api_context.hpp): what is attached to each, the slot each one's effects add into
// (oalgpu_slot_set_target), and the update's pass over them.  (Part of the C-ABI shim: see api.hip.)
#include "api_context.hpp"

static float *SlotWetBus(const DeviceLayout &L, uint32_t slot) { return L.bus + BusWetOffset(L) + size_t{slot} * L.wetChannels * kLine; }
// EffectTarget of a slot (alc/alu.cpp:627-632): its target slot's wet bus, or the device's lines (dry, then real)
static float *SlotDestination(const oalgpu_context *c, uint32_t slot)
{
    const int32_t target = c->slots[slot].target;
    return target >= 0 ? SlotWetBus(c->L, uint32_t(target)) : c->L.bus;
}
// How many lines of SlotDestination something attached to a slot may mix into, were `target` the slot's target: a wet bus's
// channels, or else the device's dry lines -- and, for a dedicated effect (realToo), the real output lines that follow them in
// the bus block.
static uint32_t SlotLineLimit(const oalgpu_context *c, int32_t target, bool realToo = false)
{
    if(target >= 0) return c->L.wetChannels;
    return c->L.numDry + (realToo ? c->L.numReal : 0u);
}

// EffectState::process of every slot that has an effect attached (alc/alu.cpp:2209-2257): from the slot's wet bus into its
// destination, on stream `s`, after the buses are final.  The slots go by descending depth (c->slotOrder, host/slot_order.cpp:
// a slot in front of the slot it targets, alu.cpp:2220-2249), so a wet bus has everything its feeders add before the slot's own
// effects read it; everything is launched on `s`, whose order is the order of the sums.  Without targets there is one depth
// and the order is the slot index.
int RunEffects(oalgpu_context *c, hipStream_t s, uint32_t samples_to_do)
{
    const DeviceLayout &L = c->L;
    for(uint32_t first = 0; first < L.numSlots; )
    {
        const uint32_t depth = c->slots[c->slotOrder[first]].depth;
        uint32_t last = first;
        while(last < L.numSlots && c->slots[c->slotOrder[last]].depth == depth) ++last;
        for(uint32_t i = first; i < last; ++i)
        {
            const uint32_t slot = c->slotOrder[i];
            const float *wet = SlotWetBus(L, slot);
            if(oalgpu_convolution *conv = c->slots[slot].conv)
            {
                if(int rc = oalgpu_convolution_process_device(conv, s, wet, SlotDestination(c, slot), samples_to_do)) return rc;
            }
            if(oalgpu_effect *fx = c->slots[slot].effect)
            {
                if(int rc = oalgpu_effect_process_device(fx, s, wet, SlotDestination(c, slot), samples_to_do)) return rc;
            }
        }
        // the EAX reverbs of the depth's slots: one launch, instances side by side, mix-out in slot order
        oalgpu_reverb *revs[kRvBatchMax];
        const float *wets[kRvBatchMax];
        float *outs[kRvBatchMax];
        uint32_t count = 0;
        auto flush = [&]() -> int
        {
            if(!count) return OALGPU_OK;
            const int rc = oalgpu_reverb_process_batch_device(revs, wets, count, outs, samples_to_do, s, c->reverbTicket.p);
            count = 0;
            return rc;
        };
        for(uint32_t i = first; i < last; ++i)
        {
            const uint32_t slot = c->slotOrder[i];
            if(!c->slots[slot].reverb) continue;
            revs[count] = c->slots[slot].reverb;
            wets[count] = SlotWetBus(L, slot);
            outs[count] = SlotDestination(c, slot);
            if(++count == kRvBatchMax) { if(int rc = flush()) return rc; }
        }
        if(int rc = flush()) return rc;
        first = last;
    }
    return OALGPU_OK;
}

uint32_t AttachedReverbs(const oalgpu_context *c)
{ return uint32_t(std::count_if(c->slots.begin(), c->slots.end(), [](const EffectSlot &s) { return s.reverb != nullptr; })); }

int oalgpu_slot_set_convolution(oalgpu_context *c, uint32_t slot, oalgpu_convolution *conv)
{
    if(!c || slot >= c->L.numSlots) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_set_convolution: bad slot");
    const int32_t target = c->slots[slot].target;
    if(conv && ConvOutLines(conv) > SlotLineLimit(c, target))
        return Fail(OALGPU_ERR_INVALID, target >= 0 ? "oalgpu_slot_set_convolution: the effect mixes into more lines than the wet bus of the slot's target has"
            : "oalgpu_slot_set_convolution: the effect mixes into more lines than the context has dry lines");
    if(int rc = oalgpu_sync(c)) return rc;
    c->slots[slot].conv = conv;
    return OALGPU_OK;
}

int oalgpu_slot_set_effect(oalgpu_context *c, uint32_t slot, oalgpu_effect *fx)
{
    if(!c || slot >= c->L.numSlots) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_set_effect: bad slot");
    // (a dedicated effect may address the real output lines, which follow the dry lines in the bus block)
    // (on a slot with a target: the target's wet bus)
    if(fx && (EffectOutLines(fx) > SlotLineLimit(c, c->slots[slot].target, true) || EffectInChannels(fx) > c->L.wetChannels))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_set_effect: the effect's lines do not fit the context's buses");
    if(int rc = oalgpu_sync(c)) return rc;
    c->slots[slot].effect = fx;
    return OALGPU_OK;
}

int oalgpu_slot_set_reverb(oalgpu_context *c, uint32_t slot, oalgpu_reverb *rev)
{
    if(!c || slot >= c->L.numSlots) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_set_reverb: bad slot");
    if(rev && c->L.wetChannels < 4)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_set_reverb: the reverb reads a 4-line B-Format wet bus");
    const int32_t target = c->slots[slot].target;
    if(rev && ReverbOutLines(rev) > SlotLineLimit(c, target))
        return Fail(OALGPU_ERR_INVALID, target >= 0 ? "oalgpu_slot_set_reverb: the effect mixes into more lines than the wet bus of the slot's target has"
            : "oalgpu_slot_set_reverb: the effect mixes into more lines than the context has dry lines");
    if(int rc = oalgpu_sync(c)) return rc;
    if(rev) { if(int rc = oalgpu_reverb_set_math_mode(rev, c->exact ? OALGPU_MATH_EXACT : OALGPU_MATH_FAST)) return rc; }
    c->slots[slot].reverb = rev;
    return RebalanceWaveGroups(c);
}

/* ---- effect slot targets: AL_EFFECTSLOT_TARGET_SOFT (al/auxeffectslot.cpp:504-520; alc/alu.cpp:627-632, :2220-2249) ---- */
int oalgpu_slot_order(const int32_t *targets, uint32_t num_slots, uint32_t *order, uint32_t *depth)
{
    if(num_slots && (!targets || !order)) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_order: null argument");
    if(!SlotOrder(targets, num_slots, order, depth))
        return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_order: a target out of range, a slot that targets itself, or a cycle");
    return OALGPU_OK;
}

int oalgpu_slot_set_target(oalgpu_context *c, uint32_t slot, int32_t target_slot)
{
    const std::string w = "oalgpu_slot_set_target: ";
    if(!c) return Fail(OALGPU_ERR_INVALID, w + "null context");
    if(slot >= c->L.numSlots) return Fail(OALGPU_ERR_INVALID, w + "bad slot");
    if(target_slot < -1 || target_slot >= int32_t(c->L.numSlots)) return Fail(OALGPU_ERR_INVALID, w + "the target is out of range (-1 .. num_slots - 1)");
    if(target_slot == int32_t(slot)) return Fail(OALGPU_ERR_INVALID, w + "a slot cannot target itself");
    // (a copy with the new target, ordered beside the old one and swapped in whole behind the checks)
    std::vector<EffectSlot> slots = c->slots;
    slots[slot].target = target_slot;
    std::vector<int32_t> targets(c->L.numSlots);
    for(uint32_t i = 0; i < c->L.numSlots; ++i) targets[i] = slots[i].target;
    std::vector<uint32_t> order(c->L.numSlots), depth(c->L.numSlots);
    if(!SlotOrder(targets.data(), c->L.numSlots, order.data(), depth.data()))
        return Fail(OALGPU_ERR_INVALID, w + "the target would close a cycle");
    for(uint32_t i = 0; i < c->L.numSlots; ++i) slots[i].depth = depth[i];
    // (towards a wet bus only: what was attached on the way to another slot is not measured against the device's lines again)
    const EffectSlot &S = slots[slot];
    if(target_slot >= 0 && (ConvOutLines(S.conv) > SlotLineLimit(c, target_slot) || EffectOutLines(S.effect) > SlotLineLimit(c, target_slot, true)
        || ReverbOutLines(S.reverb) > SlotLineLimit(c, target_slot)))
        return Fail(OALGPU_ERR_INVALID, w + "what is attached to the slot mixes into more lines than the target's wet bus has");
    if(int rc = oalgpu_sync(c)) return rc;
    c->slots.swap(slots);
    c->slotOrder.swap(order);
    return OALGPU_OK;
}

int oalgpu_slot_target(oalgpu_context *c, uint32_t slot, int32_t *target_slot)
{
    if(!c || !target_slot) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_target: null argument");
    if(slot >= c->L.numSlots) return Fail(OALGPU_ERR_INVALID, "oalgpu_slot_target: bad slot");
    *target_slot = c->slots[slot].target;
    return OALGPU_OK;
}
