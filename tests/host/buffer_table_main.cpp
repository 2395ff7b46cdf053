// The buffer table's lifetime rules at table level (openal-soft_amd/host/buffer_table.cpp), built with the address and
// undefined-behaviour sanitizers by tests/test_buffer_table_host.py: the four scenarios of tests/test_buffer_lifetime.py with
// the storage each step hands back for freeing, a queue long enough to show a recursion, and a random walk against a model
// that recomputes every reference count from scratch.
#include "../../openal-soft_amd/host/buffer_table.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

using oalgpu::BufferTable;
using Freed = std::vector<void*>;
static void Take(Freed &f, const Freed &more) { f.insert(f.end(), more.begin(), more.end()); }

#define CHECK(cond) do { if(!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } } while(0)

// oalgpu_buffer_release: refused unless the handle may still be named
static bool Release(BufferTable &t, int h, Freed &f) { if(!t.usable(h)) return false; Take(f, t.release(h)); return true; }
static void *Storage(size_t id) { return reinterpret_cast<void*>(uintptr_t{0x10000} + id * 16u); }

struct Triple { bool live, pending; uint32_t refs; };
static bool operator==(const Triple &a, const Triple &b) { return a.live == b.live && a.pending == b.pending && a.refs == b.refs; }
// what oalgpu_buffer_info reports
static Triple Info(const BufferTable &t, int h) { const auto &b = t.at(h); return Triple{b.live, b.live && b.released, b.refs}; }

static void ReleasedWhileHeld()
{
    BufferTable t; t.reset(8, 8);
    Freed f;
    const int ha = t.alloc(Storage(1), 0, -1);
    CHECK(ha == 0);
    Take(f, t.start(0, ha));
    CHECK(Release(t, ha, f) && f.empty());
    CHECK(Info(t, ha) == (Triple{true, true, 1}));           // held by the voice slot
    CHECK(!t.usable(ha));                                    // ... but no longer to be named
    CHECK(!Release(t, ha, f));                               // released before
    Take(f, t.stop(0));                                      // the slot lets go
    CHECK(f == Freed{Storage(1)});
    CHECK(!t.at(ha).live && !t.live(ha));
    CHECK(t.alloc(Storage(2), 0, -1) == ha);                 // the handle comes back
    CHECK(t.at(ha).storage == Storage(2));
}

static void FortyThroughFour()
{
    BufferTable t; t.reset(4, 8);
    Freed f;
    const int first = t.alloc(Storage(100), 0, -1);
    Take(f, t.start(0, first));
    CHECK(f.empty());
    for(size_t k = 0; k < 40; ++k)
    {
        const int h = t.alloc(Storage(k), 0, -1);
        CHECK(h >= 0 && h < 4);
        f.clear();
        Take(f, t.start(0, h));                              // the slot lets go of the buffer before: released, so it dies
        CHECK(k == 0 ? f.empty() : f == Freed{Storage(k - 1)});
        f.clear();
        CHECK(Release(t, h, f) && f.empty());                // dies when the slot is started on the next one
    }
    // the table bounds the live handles: `first` and the fortieth are, two places are left
    CHECK(!t.full() && t.alloc(Storage(200), 0, -1) >= 0 && t.alloc(Storage(201), 0, -1) >= 0);
    CHECK(t.full() && t.alloc(Storage(202), 0, -1) == -1);
}

static void QueueLinkUnqueue()
{
    BufferTable t; t.reset(8, 8);
    Freed f;
    int hs[4];
    for(int i = 0; i < 4; ++i) hs[i] = t.alloc(Storage(size_t(i)), 0, -1);
    for(int i = 0; i < 3; ++i) Take(f, t.link(hs[i], hs[i + 1]));
    Take(f, t.start(0, hs[0]));
    CHECK(Release(t, hs[0], f) && f.empty());
    CHECK(Info(t, hs[0]) == (Triple{true, true, 1}));        // the voice slot still holds the queue's head
    CHECK(!t.canUnqueue(0, 1));                              // nothing read back yet
    CHECK(t.canUnqueue(0, 0));
    t.noteQueueDone(0, 1);
    CHECK(t.canUnqueue(0, 1));
    Take(f, t.unqueue(0, 1));
    CHECK(f == Freed{Storage(0)});                           // freed while the source plays on
    CHECK(!t.at(hs[0]).live);
    CHECK(t.at(hs[1]).refs == 1);                            // the voice's new head (buffer 0's link to it went with buffer 0)
    f.clear();
    CHECK(Release(t, hs[2], f) && f.empty());                // stays while the link in front of it lives
    CHECK(Info(t, hs[2]) == (Triple{true, true, 1}));
    CHECK(!t.canUnqueue(0, 5) && !t.canUnqueue(0, 1));       // more than it has played through
    // a link taken away lets its target go; the end of the queue
    Take(f, t.link(hs[1], -1));
    CHECK((f == Freed{Storage(2)}) && t.at(hs[3]).refs == 0 && t.at(hs[3]).live);
}

static void ViewHoldsParent()
{
    BufferTable t; t.reset(8, 8);
    Freed f;
    const int h = t.alloc(Storage(7), 0, -1);
    const int view = t.alloc(nullptr, 0, h);
    CHECK(t.at(h).refs == 1 && t.at(view).parent == h);
    CHECK(Release(t, h, f) && f.empty());
    CHECK(Info(t, h) == (Triple{true, true, 1}));            // the view holds the storage
    CHECK(Release(t, view, f));
    CHECK(f == Freed{Storage(7)});                           // (the view has no storage of its own)
    CHECK(!t.at(h).live && !t.at(view).live);
}

// 100 000 linked buffers, all released, held by the head's voice slot alone: one call frees them all, in queue order
static void LongChain()
{
    constexpr uint32_t N = 100000;
    BufferTable t; t.reset(N, 1);
    Freed f;
    for(uint32_t i = 0; i < N; ++i) CHECK(t.alloc(Storage(i), 0, -1) == int(i));
    for(uint32_t i = 0; i + 1 < N; ++i) Take(f, t.link(int(i), int(i + 1)));
    Take(f, t.start(0, 0));
    for(uint32_t i = 0; i < N; ++i) CHECK(Release(t, int(i), f));
    CHECK(f.empty());
    Take(f, t.stop(0));
    CHECK(f.size() == N);
    for(uint32_t i = 0; i < N; ++i) CHECK(f[i] == Storage(i));
    for(uint32_t i = 0; i < N; ++i) CHECK(!t.at(int(i)).live && t.at(int(i)).refs == 0);
    CHECK(!t.full());
}

// ---- the random walk: the table against a model that knows no reference counts, only who points at whom ----
struct Model {
    struct Buf { bool live{false}, released{false}; int parent{-1}, next{-1}; void *storage{nullptr}; };
    std::vector<Buf> bufs;
    std::vector<int> heads;
    std::vector<uint32_t> Refs() const
    {
        std::vector<uint32_t> r(bufs.size(), 0u);
        for(int h : heads) if(h >= 0) ++r[size_t(h)];
        for(const Buf &b : bufs)
        {
            if(!b.live) continue;
            if(b.parent >= 0) ++r[size_t(b.parent)];
            if(b.next >= 0) ++r[size_t(b.next)];
        }
        return r;
    }
    // released handles nobody points at die, until none is left; their storage goes into `freed`
    void Settle(std::multiset<void*> &freed)
    {
        for(bool again = true; again;)
        {
            again = false;
            const std::vector<uint32_t> r = Refs();
            for(size_t h = 0; h < bufs.size(); ++h)
                if(bufs[h].live && bufs[h].released && r[h] == 0)
                {
                    if(bufs[h].storage) freed.insert(bufs[h].storage);
                    bufs[h] = Buf{};
                    again = true;
                }
        }
    }
    bool Reaches(int from, int to) const
    {
        for(size_t steps = 0; from >= 0 && steps <= bufs.size(); ++steps, from = bufs[size_t(from)].next)
            if(from == to) return true;
        return false;
    }
};

static void RandomWalk()
{
    constexpr uint32_t kPlaces = 8, kVoices = 4;
    BufferTable t; t.reset(kPlaces, kVoices);
    Model m; m.bufs.resize(kPlaces); m.heads.assign(kVoices, -1);
    std::mt19937 rng(20240607u);
    std::set<void*> everFreed;
    size_t nextStorage = 1, deaths = 0;
    for(int step = 0; step < 10000; ++step)
    {
        Freed f;
        const uint32_t op = rng() % 8u, h = rng() % kPlaces, g = rng() % kPlaces, v = rng() % kVoices;
        const bool usableH = m.bufs[h].live && !m.bufs[h].released;
        CHECK(t.usable(int(h)) == usableH && t.live(int(h)) == m.bufs[h].live);
        switch(op)
        {
        case 0: case 1: {   // register; a view of h where h may be named
            const bool view = op == 1 && usableH;
            void *s = view ? nullptr : Storage(nextStorage++);
            size_t liveNow = 0;
            for(const auto &b : m.bufs) liveNow += b.live;
            CHECK(t.full() == (liveNow == kPlaces));
            const int n = t.alloc(s, 0, view ? int(h) : -1);
            if(liveNow == kPlaces) { CHECK(n == -1); break; }
            CHECK(n >= 0 && uint32_t(n) < kPlaces && !m.bufs[size_t(n)].live);
            m.bufs[size_t(n)] = Model::Buf{true, false, view ? int(h) : -1, -1, s};
            break; }
        case 2: case 3:     // release
            CHECK(Release(t, int(h), f) == usableH);
            if(usableH) m.bufs[h].released = true;
            break;
        case 4:             // link h -> g, or end h's queue (no cycles: a queue is a list)
            if(!m.bufs[h].live) break;
            if(rng() % 4u == 0) { Take(f, t.link(int(h), -1)); m.bufs[h].next = -1; break; }
            if(!m.bufs[g].live || m.bufs[g].released || m.Reaches(int(g), int(h))) break;
            Take(f, t.link(int(h), int(g))); m.bufs[h].next = int(g);
            break;
        case 5:             // start
            if(!usableH) break;
            Take(f, t.start(v, int(h))); m.heads[v] = int(h);
            CHECK(!t.canUnqueue(v, 1));
            break;
        case 6:             // stop
            Take(f, t.stop(v)); m.heads[v] = -1;
            break;
        default: {          // the voice's hold moves one link on
            if(m.heads[v] < 0) break;
            t.noteQueueDone(v, 0xffffffu);
            CHECK(t.canUnqueue(v, 1));
            Take(f, t.unqueue(v, 1)); m.heads[v] = m.bufs[size_t(m.heads[v])].next;
            break; }
        }
        std::multiset<void*> want;
        m.Settle(want);
        CHECK(std::multiset<void*>(f.begin(), f.end()) == want);
        for(void *p : f) CHECK(p && everFreed.insert(p).second);      // every storage pointer is handed back once
        deaths += f.size();
        const std::vector<uint32_t> refs = m.Refs();
        size_t live = 0;
        for(uint32_t i = 0; i < kPlaces; ++i)
        {
            const auto &b = t.at(int(i));
            CHECK(b.live == m.bufs[i].live && b.refs == refs[i]);
            CHECK(b.live || (b.refs == 0 && !b.released && !b.storage));   // no handle is both free and referenced
            if(b.live) CHECK(b.released == m.bufs[i].released && b.storage == m.bufs[i].storage && b.parent == m.bufs[i].parent && b.next == m.bufs[i].next);
            live += b.live;
        }
        CHECK(live <= kPlaces);
    }
    CHECK(deaths > 500);                                             // (the walk did get somewhere)
    for(int h = 0; t.inRange(h); ++h) CHECK(everFreed.count(t.at(h).storage) == 0);       // (what the table still holds)
}

int main()
{
    ReleasedWhileHeld();
    FortyThroughFour();
    QueueLinkUnqueue();
    ViewHoldsParent();
    LongChain();
    RandomWalk();
    std::puts("buffer table: ok");
    return 0;
}
