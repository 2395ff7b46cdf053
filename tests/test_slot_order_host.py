"""Effect slot targets, host side (no GPU): oalgpu_slot_order -- the processing order and depths of a context's effect slots --
on hand-written graphs and seeded random forests, the refusals (targets out of range, self-targets, cycles), and a restatement
of the reference's slot sort (alc/alu.cpp:2220-2249: partition_copy of the slots without a target to the back, then one
std::partition of the unsorted front per sorted slot, from the back) whose groups must be the depths' sets.  The order inside
a depth is the library's own (ascending slot index); the reference's is whatever its partitions leave."""
import numpy as np
import pytest

import oalgpu


def _depths(targets):
    """the definition: 0 without a target, otherwise the target's depth + 1"""
    out = []
    for i in range(len(targets)):
        d, s = 0, i
        while targets[s] >= 0:
            s = targets[s]
            d += 1
            assert d <= len(targets)
        out.append(d)
    return out


def _forest(rng, n):
    """a random forest over n slots in a random labelling: every slot targets a slot made before it, or nothing"""
    label = rng.permutation(n)
    targets = [-1] * n
    for k in range(1, n):
        if rng.random() < 0.7:
            targets[label[k]] = int(label[rng.integers(0, k)])
    return targets


def _check(targets):
    order, depth = oalgpu.slot_order(targets)
    n = len(targets)
    order, depth = [int(v) for v in order], [int(v) for v in depth]
    assert sorted(order) == list(range(n))
    assert depth == _depths(targets)
    where = {s: k for k, s in enumerate(order)}
    for s, t in enumerate(targets):
        if t >= 0:
            assert where[s] < where[t], (targets, order)
    keys = [(-depth[s], s) for s in order]
    assert keys == sorted(keys), "descending depth, ascending slot index inside a depth"
    return order, depth


def _reference_sort(targets):
    """alu.cpp:2220-2249 over slot indices (auxslots in index order)"""
    n = len(targets)
    aux = list(range(n))[::-1]                                  # auxslots.rbegin() .. rend()
    front = [s for s in aux if targets[s] >= 0]                 # partition_copy: has_target -> from the front,
    back = [s for s in aux if targets[s] < 0]                   # the others from the back (sorted_slots.rbegin())
    slots = front + [None] * (n - len(front) - len(back)) + back[::-1]
    split = len(front)
    assert split != n, "there must be at least one slot without a target"
    nxt = n
    while split > 1:
        if nxt == split:
            break
        nxt -= 1
        head = slots[:split]
        keep = [s for s in head if targets[s] != slots[nxt]]    # std::partition(begin, split_point, not_next)
        moved = [s for s in head if targets[s] == slots[nxt]]
        slots[:split] = keep + moved
        split = len(keep)
    return slots


HAND = [
    [-1],
    [-1, -1, -1, -1],
    [1, -1],                        # 0 -> 1
    [-1, 0],                        # the feeder above its target
    [-1, 0, 0],                     # two feeders of one target
    [2, -1, 1],                     # 0 -> 2 -> 1
    [1, -1, 3, -1],                 # two chains
    [1, 2, 3, -1],                  # as long as the slots
    [-1, 0, 1, 2, 3, 4, 5, 6],
    [3, 3, 3, -1, 3, 4, 4, 0],
]


@pytest.mark.parametrize("targets", HAND, ids=[",".join(map(str, t)) for t in HAND])
def test_hand_written_graphs(targets):
    _check(targets)


def test_known_orders():
    assert [list(map(int, a)) for a in oalgpu.slot_order([1, -1])] == [[0, 1], [1, 0]]
    assert [list(map(int, a)) for a in oalgpu.slot_order([-1, 0, 0])] == [[1, 2, 0], [0, 1, 1]]
    assert [list(map(int, a)) for a in oalgpu.slot_order([2, -1, 1])] == [[0, 2, 1], [2, 0, 1]]
    assert [list(map(int, a)) for a in oalgpu.slot_order([1, -1, 3, -1])] == [[0, 2, 1, 3], [1, 0, 1, 0]]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16])
def test_no_targets_is_the_identity(n):
    order, depth = oalgpu.slot_order([-1] * n)
    assert list(order) == list(range(n)) and not depth.any()


def test_no_slots():
    order, depth = oalgpu.slot_order([])
    assert order.size == 0 and depth.size == 0


def test_random_forests_and_the_reference_partition():
    rng = np.random.default_rng(2209)
    for case in range(400):
        n = int(rng.integers(1, 17))
        targets = _forest(rng, n)
        order, depth = _check(targets)
        ref = _reference_sort(targets)
        assert sorted(ref) == list(range(n)), (targets, ref)
        # the same sets per depth, in the same places: the deepest group first
        at = 0
        for d in range(max(depth), -1, -1):
            group = {s for s in range(n) if depth[s] == d}
            assert set(ref[at:at + len(group)]) == group == set(order[at:at + len(group)]), (targets, ref, order)
            at += len(group)


def _cycle(n, length):
    """slots 0 .. length-1 in a ring, the others feed it or nothing"""
    targets = [-1] * n
    for k in range(length):
        targets[k] = (k + 1) % length
    for k in range(length, n):
        targets[k] = k - 1 if k % 2 else -1
    return targets


@pytest.mark.parametrize("n,length", [(1, 1), (4, 1), (2, 2), (5, 2), (3, 3), (8, 3), (4, 4), (16, 16), (16, 5)])
def test_cycles_are_refused(n, length):
    targets = _cycle(n, length)
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.slot_order(targets)
    # the same graph with the ring opened is accepted
    targets[0] = -1
    _check(targets)


def test_a_cycle_behind_a_chain_is_refused():
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.slot_order([1, 2, 3, 1])                 # 0 -> 1 -> 2 -> 3 -> 1
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.slot_order([-1, 0, 3, 2])                # a chain beside a ring


@pytest.mark.parametrize("targets", [[1], [-2], [-1, 2], [4, -1, -1, -1], [-1, -1, -5], [2**31 - 1, -1]])
def test_targets_out_of_range_are_refused(targets):
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.slot_order(targets)


def test_a_refusal_writes_nothing_and_null_arguments_are_refused():
    import ctypes as C
    lib = oalgpu.lib
    u32 = C.POINTER(C.c_uint32)
    lib.oalgpu_slot_order.argtypes = [C.POINTER(C.c_int32), C.c_uint32, u32, u32]
    t = (C.c_int32 * 3)(1, 2, 0)
    order = (C.c_uint32 * 3)(9, 9, 9)
    depth = (C.c_uint32 * 3)(9, 9, 9)
    assert lib.oalgpu_slot_order(t, 3, order, depth) < 0
    assert list(order) == [9, 9, 9] and list(depth) == [9, 9, 9]
    t = (C.c_int32 * 3)(-1, 0, 1)
    assert lib.oalgpu_slot_order(None, 3, order, depth) < 0
    assert lib.oalgpu_slot_order(t, 3, None, depth) < 0
    assert lib.oalgpu_slot_order(t, 3, order, None) == 0        # the depths are optional
    assert list(order) == [2, 1, 0]
