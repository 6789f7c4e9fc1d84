// handoff_model.cpp -- host-thread model of the per-slot s_wait word of the streaming schedule (csrc/er_stream.hip) and of the results that
// travel beside it since ER_STREAM_LDS_HANDOFF: the winner of a closest-hit ray in the slot's s_hit word, a certain shadow verdict as a flag
// of s_wait, and -- flagged -- a second candidate (ST_HIT2) or the candidates of an ambiguous verdict (ST_AMB1 / ST_AMB2) in the slot's record.
//
// The rule under test: a tracer publishes RESULT, THEN COUNT (its add to s_wait: flags - 1), and the one whose add takes the count to zero
// appends the slot to the shade ring; a shader wave reads COUNT (the word, after it was given the slot by the ring), THEN RESULT.  The words
// a result travels through are PLAIN memory here, as on the device: only the add and the ring (csrc/er_ring.h, the kernel's own functions,
// compiled with -DER_RING_HOST_MODEL) order them, so ThreadSanitizer (tests/test_stream_handoff_cpu.py builds this with -fsanitize=thread)
// reports a hand-off the protocol leaves unordered.  Every step of a slot has its own expected results (a hash of slot, step and ray kind),
// so a consumer that sees the result of an earlier step than the one its count belongs to is caught by value: "stale".
//
//   handoff_model <slots> <steps per slot> <tracers> <shaders> [variant]
//     variant 0  the kernel's order
//     variant 1  negative control under threads: tracers add to s_wait BEFORE they write the result (timing-dependent: informational)
//   handoff_model script
//     the same negative control as ONE scripted interleaving on one thread: the shader reads between the add and the result.
//     Exit code 0 = the model caught the stale result.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../elevenrender_amd/csrc/er_ring.h"

namespace {

// the fields of a slot's s_wait word (csrc/er_stream.hip ST_*; tests/test_stream_handoff_cpu.py compares the values with the kernel's)
constexpr uint32_t COUNT_MASK = 0xFFu, FIN = 0x100u, ESC = 0x200u, AMB1 = 0x400u, AMB2 = 0x800u, OCC1 = 0x1000u, OCC2 = 0x2000u, HIT2 = 0x4000u;
static_assert((COUNT_MASK & (FIN | ESC | AMB1 | AMB2 | OCC1 | OCC2 | HIT2)) == 0u, "the flags lie above the in-flight count");
constexpr uint32_t SLOT_BITS = 11;      // as ST_SLOT_BITS: ring payload = local slot | kind << 11
constexpr int LANES = 4;

uint32_t hash32(uint32_t a) { a ^= a >> 16; a *= 0x7feb352dU; a ^= a >> 15; a *= 0x846ca68bU; a ^= a >> 16; return a; }
// what step `step` of slot `slot` is about: which rays it queues and what each of them finds
struct Plan {
    bool closest, sh1, sh2;           // rays queued (at least one)
    int hit, hit2;                    // closest: winner (-1: none), second candidate (-1: none, the common case)
    int v1, v2;                       // shadow verdicts 0 .. 3 (2, 3: ambiguous, candidates in the record)
    int a1, b1, a2, b2;               // ... their candidates
};
Plan plan_of(uint32_t slot, uint32_t step) {
    const uint32_t h = hash32(slot * 0x9E3779B9u + step * 0x85EBCA6Bu + 1u);
    Plan p;
    p.closest = (h & 7u) != 0u;
    p.sh1 = (h >> 3 & 3u) != 0u;
    p.sh2 = (h >> 5 & 3u) == 1u;
    if (!p.closest && !p.sh1 && !p.sh2) p.sh1 = true;
    const uint32_t k = hash32(h);
    p.hit = (k & 15u) == 0u ? -1 : (int)(k >> 8);                                     // one ray in sixteen leaves the scene
    p.hit2 = (p.hit >= 0 && (k >> 4 & 7u) == 0u) ? ((k >> 7 & 1u) ? -2 : (int)(hash32(k) >> 8)) : -1;      // one in eight: second candidate or overflow
    const uint32_t s = hash32(k + 1u);
    p.v1 = (s & 7u) == 0u ? 2 + (int)(s >> 3 & 1u) : (int)(s >> 4 & 1u);              // one in eight ambiguous
    p.v2 = (s >> 8 & 7u) == 0u ? 2 + (int)(s >> 11 & 1u) : (int)(s >> 12 & 1u);
    p.a1 = (int)(hash32(s + 2u) >> 8); p.b1 = (int)(hash32(s + 3u) >> 8);
    p.a2 = (int)(hash32(s + 4u) >> 8); p.b2 = (int)(hash32(s + 5u) >> 8);
    return p;
}

struct Slot {
    // LDS on the device
    uint32_t wait = 0;                // the s_wait word: atomic adds by tracers (er_ring_add), plain store by the shader that queues the rays
    int hit = 0;                      // s_hit: PLAIN
    // the slot's record (device memory): PLAIN
    int hit2 = 0, occluded[2] = {0, 0}, occ_a[2] = {0, 0}, occ_b[2] = {0, 0};
    uint32_t step = 0;                // the step whose rays are in flight (plain: written by the shader that queues them, read by tracers after the ray ring)
};

struct Ring {
    std::vector<uint32_t> cells;
    alignas(8) uint32_t ctl[ER_RING_WORDS] = {0, 0, 0, 0};
    uint32_t log2 = 0;
    void init(uint32_t l2) { log2 = l2; cells.assign(1u << l2, 0u); }
};

struct Model {
    std::vector<Slot> slots;
    Ring rays, shade;
    uint32_t steps = 0;
    int variant = 0;
    std::atomic<uint32_t> live{0};
    std::atomic<bool> done{false};
    std::atomic<uint32_t> stale{0}, bad_word{0}, guard{0}, traced{0}, shaded{0}, through_record{0};
};

void push(Model& M, Ring& R, const uint32_t* payload, uint32_t n) {
    if (n == 0) return;
    const uint32_t base = er_ring_reserve(R.ctl, n);
    for (uint32_t i = 0; i < n; i++)
        if (!er_ring_put(R.cells.data(), R.log2, base + i, payload[i])) M.guard++;
    er_ring_publish(R.ctl, n);
}
uint32_t take(Model& M, Ring& R, uint32_t* payload, uint32_t want) {
    uint32_t base = 0;
    const uint32_t g = er_ring_grant(R.ctl, want, base);
    for (uint32_t i = 0; i < g; i++)
        if (!er_ring_get(R.cells.data(), R.log2, base + i, payload[i])) M.guard++;
    return g;
}

// a shader lane queues the rays of the slot's next step: the count first (plain: nobody else touches the word now), then the rays
void queue_step(Model& M, uint32_t s, uint32_t step) {
    Slot& S = M.slots[s];
    const Plan p = plan_of(s, step);
    S.step = step;
    S.wait = (p.closest ? 1u : 0u) + (p.sh1 ? 1u : 0u) + (p.sh2 ? 1u : 0u) + (p.closest ? 0u : FIN);
    uint32_t e[3], n = 0;
    if (p.closest) e[n++] = s;
    if (p.sh1) e[n++] = s | (1u << SLOT_BITS);
    if (p.sh2) e[n++] = s | (2u << SLOT_BITS);
    push(M, M.rays, e, n);
}

// what a tracer lane does at its publish (er_stream.hip, tracer_publish): result, then count; returns true if it was the slot's last ray
bool publish(Model& M, uint32_t e, uint32_t& fin) {
    const uint32_t s = e & ((1u << SLOT_BITS) - 1u), kind = e >> SLOT_BITS;
    Slot& S = M.slots[s];
    const Plan p = plan_of(s, S.step);
    uint32_t flags = 0;
    auto result = [&] {
        if (kind == 0u) {
            S.hit = p.hit;
            if (p.hit2 != -1) { S.hit2 = p.hit2; M.through_record++; }
        } else {
            const int v = kind == 1u ? p.v1 : p.v2;
            if (v >= 2) {
                S.occluded[kind - 1u] = v;
                S.occ_a[kind - 1u] = kind == 1u ? p.a1 : p.a2;
                S.occ_b[kind - 1u] = kind == 1u ? p.b1 : p.b2;
                M.through_record++;
            }
        }
    };
    if (kind == 0u) flags = (p.hit < 0 ? ESC : 0u) | (p.hit2 != -1 ? HIT2 : 0u);
    else {
        const int v = kind == 1u ? p.v1 : p.v2;
        flags = v >= 2 ? (kind == 1u ? AMB1 : AMB2) : (v == 1 ? (kind == 1u ? OCC1 : OCC2) : 0u);
    }
    if (M.variant == 0) result();
    const uint32_t add = flags - 1u;
    fin = er_ring_add(&S.wait, add) + add;
    if (M.variant != 0) result();      // (the negative control's order)
    M.traced++;
    return (fin & COUNT_MASK) == 0u;
}

// what a shader lane reads when the shade ring gives it the slot: the word, then the results the word says are there
void check_step(Model& M, uint32_t s) {
    Slot& S = M.slots[s];
    const Plan p = plan_of(s, S.step);
    const uint32_t w = S.wait;
    uint32_t want = p.closest ? 0u : FIN;
    if (p.closest) want |= (p.hit < 0 ? ESC : 0u) | (p.hit2 != -1 ? HIT2 : 0u);
    if (p.sh1) want |= p.v1 >= 2 ? AMB1 : (p.v1 == 1 ? OCC1 : 0u);
    if (p.sh2) want |= p.v2 >= 2 ? AMB2 : (p.v2 == 1 ? OCC2 : 0u);
    if (w != want) M.bad_word++;
    if (p.closest) {
        if (S.hit != p.hit) M.stale++;
        if ((w & HIT2) && S.hit2 != p.hit2) M.stale++;
    }
    if (p.sh1 && (w & AMB1) && (S.occluded[0] != p.v1 || S.occ_a[0] != p.a1 || S.occ_b[0] != p.b1)) M.stale++;
    if (p.sh2 && (w & AMB2) && (S.occluded[1] != p.v2 || S.occ_a[1] != p.a2 || S.occ_b[1] != p.b2)) M.stale++;
    M.shaded++;
}

void tracer(Model& M) {
    uint32_t e[LANES];
    while (!M.done.load(std::memory_order_acquire)) {
        const uint32_t g = take(M, M.rays, e, LANES);
        if (g == 0) { er_ring_pause(); continue; }
        // (a wave publishes its lanes' rays together: all the adds, then one push for the slots that are complete)
        uint32_t out[LANES], n = 0;
        for (uint32_t i = 0; i < g; i++) {
            uint32_t fin = 0;
            if (publish(M, e[i], fin)) out[n++] = e[i] & ((1u << SLOT_BITS) - 1u);
        }
        push(M, M.shade, out, n);
    }
}

void shader(Model& M) {
    uint32_t e[LANES];
    while (!M.done.load(std::memory_order_acquire)) {
        const uint32_t g = take(M, M.shade, e, LANES);
        if (g == 0) { er_ring_pause(); continue; }
        for (uint32_t i = 0; i < g; i++) {
            check_step(M, e[i]);
            const uint32_t next = M.slots[e[i]].step + 1u;
            if (next < M.steps) queue_step(M, e[i], next);
            else if (M.live.fetch_sub(1u, std::memory_order_acq_rel) == 1u) M.done.store(true, std::memory_order_release);
        }
    }
}

// the negative control as ONE scripted interleaving on one thread: a tracer that adds before it writes, a shader that reads in between
int script() {
    Model M;
    M.slots.resize(1);
    M.rays.init(2); M.shade.init(2);
    M.steps = 64;
    int caught = 0;
    for (uint32_t step = 0; step < M.steps; step++) {
        // a step with a closest-hit ray only, so that the add takes the count to zero at once
        Slot& S = M.slots[0];
        S.step = step;
        const Plan p = plan_of(0, step);
        if (!p.closest || p.sh1 || p.sh2) continue;
        S.wait = 1u;
        const uint32_t flags = (p.hit < 0 ? ESC : 0u) | (p.hit2 != -1 ? HIT2 : 0u), add = flags - 1u;
        const uint32_t fin = er_ring_add(&S.wait, add) + add;          // count ...
        const uint32_t before = M.stale.load();
        if ((fin & COUNT_MASK) == 0u) check_step(M, 0);                // ... the shader reads here ...
        S.hit = p.hit; S.hit2 = p.hit2;                                // ... and only now the result
        if (M.stale.load() != before) caught++;
    }
    printf("count-then-result, scripted: the shader saw a stale result in %d steps\n", caught);
    return caught > 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "script") return script();
    if (argc < 5) { fprintf(stderr, "usage: handoff_model <slots> <steps per slot> <tracers> <shaders> [variant] | script\n"); return 2; }
    Model M;
    const uint32_t slots = (uint32_t)atoi(argv[1]);
    M.steps = (uint32_t)atoi(argv[2]);
    const int tracers = atoi(argv[3]), shaders = atoi(argv[4]);
    M.variant = argc > 5 ? atoi(argv[5]) : 0;
    if (slots < 1 || slots > (1u << SLOT_BITS) || M.steps < 1 || tracers < 1 || shaders < 1) { fprintf(stderr, "refused: bad arguments\n"); return 2; }
    M.slots.resize(slots);
    // (as on the device the rings hold everything that can be in flight: three rays per slot, every slot once)
    uint32_t l2 = 2;
    while ((1u << l2) < 3u * slots || (1u << l2) < 4u * LANES) l2++;
    M.rays.init(l2); M.shade.init(l2);
    M.live.store(slots);
    for (uint32_t s = 0; s < slots; s++) queue_step(M, s, 0);
    std::vector<std::thread> th;
    for (int i = 0; i < tracers; i++) th.emplace_back(tracer, std::ref(M));
    for (int i = 0; i < shaders; i++) th.emplace_back(shader, std::ref(M));
    for (auto& t : th) t.join();
    const bool empty = M.rays.ctl[ER_RING_COUNT] == 0 && M.shade.ctl[ER_RING_COUNT] == 0;
    printf("slots %u, steps %u: rays traced %u, steps shaded %u (want %u), results through the record %u, stale results %u, wrong words %u, guards %u, rings %s\n", slots,
           M.steps, M.traced.load(), M.shaded.load(), slots * M.steps, M.through_record.load(), M.stale.load(), M.bad_word.load(), M.guard.load(), empty ? "empty" : "NOT empty");
    const bool ok = M.shaded.load() == slots * M.steps && M.stale.load() == 0 && M.bad_word.load() == 0 && M.guard.load() == 0 && empty && M.through_record.load() > 0;
    return ok ? 0 : 1;
}
