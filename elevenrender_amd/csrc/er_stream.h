// er_stream.h -- launch wrapper of the CU-resident streaming schedule (er_stream.hip, ER_FLAG_STREAM).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

struct DevScene;

#ifndef ER_STREAM_SLOTS
#define ER_STREAM_SLOTS 1024u     // slots (pixels in flight) per workgroup; one workgroup of 16 waves per CU.  Measured on C2 with the
                                  // top of the tree in LDS: 768 -> 1060, 1024 -> 1330, 1536 -> 1311, 2048 -> 1286 Msamples/s (the LDS the
                                  // rings of more slots take is worth more as tree levels)
#endif

#ifndef ER_STREAM_SUPER_TILE_DEFAULT
#define ER_STREAM_SUPER_TILE_DEFAULT 8u   // side of the screen regions dealt whole to one XCD, in tiles: the deal that spreads a frame's cost evenly
#endif
#ifndef ER_STREAM_SUPER_TILE_LARGE
#define ER_STREAM_SUPER_TILE_LARGE 16u    // the deal a render moves to after its first call if the frame's cost is even: an XCD's 512 tiles in flight are two compact regions
                                          // instead of eight, +1.6 % on C2, +5 % on C4, +2.5 % on C5 (frames of even cost) -- and -8 ... -18 % on frames whose cost is uneven
                                          // (the soup seen from far away / off to one side: fewer, larger regions per XCD sample the cost too coarsely), so the library
                                          // takes it only if the XCDs' shares of the work COUNTED during the first call (path lengths per tile) are within
                                          // ER_STREAM_COST_SPREAD_MAX of each other under it (er_stream_host.cpp stream_adapt; profiles/r04_sweep_super_tile.log, r05_deal_by_counted_work.log)
#endif
#ifndef ER_STREAM_COST_SPREAD_MAX
#define ER_STREAM_COST_SPREAD_MAX 0.04    // (max - min) / mean of the eight XCDs' summed path lengths under the large deal: 0.011 C4, 0.019 Cornell at 1080p, 0.021 C2 (large regions +0.6 ... +4 %); 0.125 / 0.40 on the soup off to one side / from far away (large regions -8 % / -18 %)
#endif
#ifndef ER_STREAM_ADAPT_MIN_MS
#define ER_STREAM_ADAPT_MIN_MS 4.0       // a launch shorter than this (device time) is no reading of the tracer lanes' occupancy: start-up and tail dominate it
#endif
#ifndef ER_STREAM_SMALL_SHARE
#define ER_STREAM_SMALL_SHARE 1152u  // owned pixels per CU up to which a workgroup runs as 12 waves of 168 registers (9 tracers + 3 shaders) instead of 16 of 128
#endif
#ifndef ER_STREAM_TEN_TRACERS_SHARE
#define ER_STREAM_TEN_TRACERS_SHARE 704u   // ... of which 10 trace above this many owned pixels per CU, 9 up to it
#endif
#ifndef ER_STREAM_SPEC_SHARE
#define ER_STREAM_SPEC_SHARE 2304u   // owned pixels per CU up to which the kernel's form with speculative samples is launched (`spec`; the 12-wave form always is)
#endif
#ifndef ER_STREAM_SPEC_MIN_TRIS
#define ER_STREAM_SPEC_MIN_TRIS 1000u   // scenes of fewer triangles never start speculative samples (er_stream.hip ST_DRAWS_MASK; C1: -9 % with them)
#endif
#ifndef ER_STREAM_SPEC_LONG_DEFAULT
#define ER_STREAM_SPEC_LONG_DEFAULT 12  // sixteenths of max_bounces: pixels whose paths are longer than that on average start a speculative successor with every sample
#endif
#ifndef ER_STREAM_KEEP_SHARE
#define ER_STREAM_KEEP_SHARE 6000u   // owned pixels per CU up to which the kernel's form is launched in which a pixel that is behind its workgroup's most advanced one keeps
                                     // its slot (er_stream.hip s_front): C2's 1/2 and 1/3 shares 3 ... 5 % faster, a 200 000-triangle soup at 1280 x 720 (3 600 pixels per
                                     // CU) 4.6 %; the whole C2 frame (8 100) +- 0.5 %: it stays in the plain form, the code of round 5
#endif
#ifndef ER_STREAM_SPEC_KEEP_DEFAULT
#define ER_STREAM_SPEC_KEEP_DEFAULT 2   // 1 + the samples a pixel may be behind its workgroup's most advanced one before it goes on in the slot it has (0 = off)
#endif
#define ER_STREAM_MAX_RING 32768u  // cells of a workgroup's pixel ring at most (one "entry read" bit per cell in LDS): a rank may own
                                  // up to 256 x 32768 = 8.4 M pixels under this schedule (a 4K frame), beyond that er_render_begin takes the wavefront one

// The control words the kernel and the host share, as indices from the `status` pointer the kernel is given.  The launch adds up
// the 64-bit counts with 64-bit atomics, which need an address that is 0 (mod 8): they start at status + 1, so `status` itself sits
// on an ODD word -- the host's buffer has ER_STREAM_CTL_LEAD unused words in front of it.  The caller of a launch zeroes everything from
// ER_SC_ITERS on and sets ER_SC_START to all ones (a minimum); ER_SC_STATUS stays set until the next er_render_begin.
enum ErStreamCtl : uint32_t {
    ER_SC_STATUS = 0,     // 0 unless a wave's watchdog or a ring guard fired (bits: er_stream.hip ST_ERR_*)
    ER_SC_ITERS = 1,      // 64 bit: iterations of all tracer waves' loops ...
    ER_SC_BUSY = 3,       // 64 bit: ... and the lanes that held a ray in them
    ER_SC_START = 5,      // 64 bit: the earliest start of a workgroup, wall_clock64() ticks (100 MHz)
    ER_SC_END = 7,        // 8 x 64 bit: [+ 2 x] the latest end of a wave of XCD x = workgroup index % 8
    ER_SC_SPEC = 23,      // speculative samples started, [+ 1] whose guess was right, [+ 2] wrong
    ER_SC_WORDS = 26,     // one past the last of the words above
    ER_SC_WG_END = 27     // blocks x 64 bit behind them (one word of padding: 8-byte aligned): [+ 2 b] the latest end of a wave of workgroup b
};
constexpr uint32_t ER_STREAM_CTL_LEAD = 1;      // words of the host's buffer in front of `status` (a count, not an index from it)
static_assert((ER_STREAM_CTL_LEAD + ER_SC_ITERS) % 2u == 0u && ER_SC_BUSY % 2u == 1u && ER_SC_START % 2u == 1u && ER_SC_END % 2u == 1u && ER_SC_WG_END % 2u == 1u && ER_SC_WG_END >= ER_SC_WORDS,
              "the 64-bit control words are 8-byte aligned");
constexpr uint32_t er_stream_ctl_words(uint32_t blocks) { return ER_SC_WG_END + 2u * blocks; }      // how many words `status` points at

// One launch of the streaming kernel.  S_dev: a device copy of S (the kernel reads the scene descriptor from constant memory, not
// from its arguments).  ER_FLAG_MESH_LIGHTS (er_mesh_active): er_launch_stream hands the launch to er_launch_stream_mesh (er_stream_mesh.hip).
struct ErStreamLaunch {
    const DevScene* S = nullptr;        // host copy of the scene descriptor ...
    const DevScene* S_dev = nullptr;    // ... and its device copy
    void* records = nullptr;            // slots * er_stream_record_bytes(lights) bytes
    uint32_t slots = 0;                 // blocks * ER_STREAM_SLOTS
    bool lights = false;                // the records carry a light query's line (point lights or emitters)
    void* spill = nullptr;              // er_stream_spill_entries(blocks) uint2 entries
    const uint32_t* deal = nullptr;     // device copy of er_stream_deal_tiles' `out` ...
    uint32_t deal_count = 0;            // ... and its size
    void* ring = nullptr;               // the workgroups' pixel rings: blocks * ring_cap uint2 entries
    uint32_t ring_cap = 0;              // a power of two >= 64 * the deal's largest share and <= ER_STREAM_MAX_RING
    uint32_t* status = nullptr;         // er_stream_ctl_words(blocks) control words (ErStreamCtl)
    uint32_t n_samples = 0;
    bool count = false;                 // the instrumented instances of ER_FLAG_COUNTERS
    uint32_t blocks = 0;                // workgroups: one per CU
    uint32_t tracers = 0;               // waves that trace, of ...
    uint32_t waves = 16;                // ... 16 (1024 threads, 128 registers per wave) or 12 (768 threads, 168 registers) per workgroup
    bool spec = false;                  // the share is small enough for speculative samples ...
    bool keep = false;                  // ... for the keep rule (what is launched: er_stream_launch_form)
    hipStream_t stream = nullptr;
};
void er_launch_stream_mesh(const ErStreamLaunch& L);
void er_launch_stream(const ErStreamLaunch& L);
// The kernel form a launch uses: 0 plain, 1 with the keep rule, 2 with that and speculative samples; at 12 or 16 waves; `bits` is
// what the form adds to the kernel's last argument.  One function for the launcher and for what er_debug_stream_info reports; it
// honours the launcher's A/B knobs (ER_STREAM_SPEC, _SPEC_SLACK, _SPEC_LONG, _SPEC_KEEP; read once per process).
struct ErStreamLaunchForm { uint32_t form, waves, bits; };
ErStreamLaunchForm er_stream_launch_form(uint32_t max_bounces, uint32_t tri_count, uint32_t waves, bool spec, bool keep);
// the deal of the owned tiles to the workgroups (er_stream_host.cpp; device copy of `out` = ErStreamLaunch::deal, deal_count = out.size()); returns the most tiles of one workgroup
// edge: side of a super-tile in 8 x 8 tiles; 0 = ER_STREAM_SUPER_TILE from the environment, else ER_STREAM_SUPER_TILE_DEFAULT
uint32_t er_stream_deal_tiles(const uint32_t* owned, uint32_t count, uint32_t tiles_x, uint32_t blocks, bool xcd_aware, std::vector<uint32_t>& out, uint32_t edge = 0);
// The deal `deal` (of `blocks` workgroups, as er_stream_deal_tiles made it) levelled by counted cost (er_stream_host.cpp): cost[t] = the
// counted work of tile t of the frame (tiles beyond cost_n count 0), cap = the most tiles a workgroup may get.  Same layout; returns the
// most tiles of one workgroup.  Pure and deterministic; a total cost of 0 gives `deal` back.
uint32_t er_stream_level_by_cost(const std::vector<uint32_t>& deal, uint32_t tiles_x, uint32_t blocks, const uint32_t* cost, size_t cost_n, uint32_t cap, std::vector<uint32_t>& out);
uint32_t er_stream_record_bytes(bool lights);
size_t er_stream_spill_entries(uint32_t blocks);
hipError_t er_probe_stream(const char** which);
