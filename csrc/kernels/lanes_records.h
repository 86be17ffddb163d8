// Host <-> device records of the lanes loops (lanes_kernels.h), without any HIP
// include: the host protocol of the asynchronous lanes (csrc/host/lanes_protocol.h)
// and its CPU self-test fill and read them with a plain C++ compiler.
#pragma once
#include <cstddef>
#include <type_traits>

#ifndef PSX_HD
#if defined(__HIPCC__)
#define PSX_HD __host__ __device__
#else
#define PSX_HD
#endif
#endif

namespace psx {

// Per-round arguments of one lane: the window and the new rows of this round:
// dataset rows first + i * step (i < n) into ring slots (dst + i) % cap, then (a
// delivery that wraps the worker's shard) first2 + i * step (i < n2) into slots
// (dst + n + i) % cap.
struct LaneRound {
  int B, start, n, dst;
  long long first, step, first2;
  int n2;
  int delay_us;  // BSP round kernel: injected straggler delay before the lane's solve (0: none)
};

// Host <-> device records are 16-B chunks {tag, 3 x u32 payload}: a chunk is
// written by ONE 16-B store, so a reader that sees every chunk carry the
// expected tag has the whole record, without ordering between the stores.
struct alignas(16) TagChunk {
  unsigned tag, a, b, c;
};
constexpr int kRelChunks = 8;
struct alignas(16) AsyncRelease {  // host -> lane (pinned), tag = the lane's record count
  TagChunk ch[kRelChunks];
};
// release record payload (unpacked on both sides by the same layout)
struct RelRec {
  int stop;              // 1: leave the launch (no solve)
  long long vc;          // the pulled weights' version (tracker clock)
  long long snap;        // ticket whose snapshot holds the pulled weights
  LaneRound r;           // window + this solve's new stream rows
  unsigned long long slot_w, slot_s;  // pinned EvalSlot addresses (0: no row)
  unsigned seq_w, seq_s;              // their sequence numbers (low 32 bits)
  int delay_us;          // injected straggler delay before the push (tests)
  unsigned pull_tag;     // peer data plane: the receive slot's tag that carries these weights
};
PSX_HD inline void pack_release(const RelRec& q, unsigned tag, TagChunk* ch) {
  auto lo = [](long long v) { return (unsigned)(unsigned long long)v; };
  auto hi = [](long long v) { return (unsigned)((unsigned long long)v >> 32); };
  ch[0] = TagChunk{tag, (unsigned)q.stop, lo(q.vc), hi(q.vc)};
  ch[1] = TagChunk{tag, lo(q.snap), hi(q.snap), (unsigned)q.r.B};
  ch[2] = TagChunk{tag, (unsigned)q.r.start, (unsigned)q.r.n, (unsigned)q.r.dst};
  ch[3] = TagChunk{tag, lo(q.r.first), hi(q.r.first), (unsigned)q.r.n2};
  ch[4] = TagChunk{tag, lo(q.r.step), hi(q.r.step), lo(q.r.first2)};
  ch[5] = TagChunk{tag, hi(q.r.first2), lo((long long)q.slot_w), hi((long long)q.slot_w)};
  ch[6] = TagChunk{tag, q.seq_w, lo((long long)q.slot_s), hi((long long)q.slot_s)};
  ch[7] = TagChunk{tag, q.seq_s, (unsigned)q.delay_us, q.pull_tag};
}
PSX_HD inline void unpack_release(const TagChunk* ch, RelRec& q) {
  auto j = [](unsigned l, unsigned h) { return (long long)(((unsigned long long)h << 32) | l); };
  q.stop = (int)ch[0].a;
  q.vc = j(ch[0].b, ch[0].c);
  q.snap = j(ch[1].a, ch[1].b);
  q.r.B = (int)ch[1].c;
  q.r.start = (int)ch[2].a;
  q.r.n = (int)ch[2].b;
  q.r.dst = (int)ch[2].c;
  q.r.first = j(ch[3].a, ch[3].b);
  q.r.n2 = (int)ch[3].c;
  q.r.step = j(ch[4].a, ch[4].b);
  q.r.first2 = j(ch[4].c, ch[5].a);
  q.slot_w = (unsigned long long)j(ch[5].b, ch[5].c);
  q.seq_w = ch[6].a;
  q.slot_s = (unsigned long long)j(ch[6].b, ch[6].c);
  q.seq_s = ch[7].a;
  q.delay_us = (int)ch[7].b;
  q.pull_tag = ch[7].c;
  q.r.delay_us = 0;
}
// token: lane -> host (pinned ring, slot t % ring): {tag = ticket (low 32 bits,
// tickets start at 1), lane, vc low, vc high}
typedef TagChunk AsyncToken;

// The kernels read these through byte offsets (16-B chunk loads, the tag first) and
// take LaneRound by value inside their argument blocks: the layouts are fixed.
static_assert(std::is_trivially_copyable<RelRec>::value && std::is_standard_layout<RelRec>::value, "RelRec");
static_assert(sizeof(TagChunk) == 16 && alignof(TagChunk) == 16 && offsetof(TagChunk, tag) == 0 &&
                  offsetof(TagChunk, a) == 4 && offsetof(TagChunk, b) == 8 && offsetof(TagChunk, c) == 12,
              "TagChunk: one 16-B store, the tag first");
static_assert(sizeof(AsyncRelease) == 16 * kRelChunks && alignof(AsyncRelease) == 16, "AsyncRelease");
static_assert(sizeof(LaneRound) == 48 && offsetof(LaneRound, B) == 0 && offsetof(LaneRound, start) == 4 &&
                  offsetof(LaneRound, n) == 8 && offsetof(LaneRound, dst) == 12 && offsetof(LaneRound, first) == 16 &&
                  offsetof(LaneRound, step) == 24 && offsetof(LaneRound, first2) == 32 &&
                  offsetof(LaneRound, n2) == 40 && offsetof(LaneRound, delay_us) == 44,
              "LaneRound");
static_assert(sizeof(RelRec) == 104 && offsetof(RelRec, vc) == 8 && offsetof(RelRec, snap) == 16 &&
                  offsetof(RelRec, r) == 24 && offsetof(RelRec, slot_w) == 72 && offsetof(RelRec, slot_s) == 80 &&
                  offsetof(RelRec, seq_w) == 88 && offsetof(RelRec, seq_s) == 92 && offsetof(RelRec, delay_us) == 96 &&
                  offsetof(RelRec, pull_tag) == 100,
              "RelRec");

}  // namespace psx
