// Host side of the relay (kernels.h: relay_begin / relay_end; profiles/r05_relay_segments.txt): a launch's steps cut into
// segments that are handed from workgroup to workgroup inside the launch, so that a CU that is free takes the next (segment,
// chain block) in line instead of idling behind a slower one.  Everything the host does for it is here, and everything travels
// in arguments: an entry point (arp_api.hip) asks with relay_prepare, which fills a RelayAsk -- one zeroed flag word per chain
// block that belongs to THIS launch alone, a stream-ordered allocation, so launches of one handle that overlap on different
// streams never share a word; the launcher (host_common.h) knows its kernel and decides with relay_plan, the one place that
// writes the seg_* fields of the parameters a kernel gets, and returns what it decided as a RelayGeometry; relay_release
// gives the allocation back behind the launch.  No HIP kernel and nothing of the model handle in here.
// Experiments (ARP_DEBUG=1 only): ARP_SEGMENTS=n forces the count, ARP_SEGMENT_RATIO=percent the taper, ARP_SEGMENT_LENS=
// n0,n1,... both, as explicit lengths (of a launch of any length; the others cut launches from 256 steps on); ARP_RELAY_PUBLISH=
// fence|through and ARP_RELAY_ACQUIRE=wave|group choose the hand-over's form; ARP_RELAY_TIMEOUT_MS and ARP_RELAY_FAULT=1 bring
// the failure path on demand.
#pragma once
#include <map>
#include <mutex>
#include <vector>
#include "host_error.h"
#include "kernels.h"

namespace arp {

// what a chain launch did (arp_relay_geometry, a measurement hook): segments, chain blocks, workgroups of the kernel one CU
// holds (0 where the launcher did not have to ask)
struct RelayGeometry { int v[3]; };
// The cut of a launch's n_steps into `segs` segments (1 <= segs <= n_steps), lengths proportional to ratio^s: a free slot
// takes the next (segment, block) in line, so the launch ends with slots idle for about half a last-round segment -- a short
// last round leaves a short tail, and the hand-overs stay `segs` per block (profiles/r07_relay_schedule.txt).  Every
// segment gets one step, the rest goes out in proportion (rounded down), what the rounding leaves to the first segments:
// the lengths sum to n_steps, never increase and are all >= 1.  ratio = 1 is the equal cut as it has always been,
// ceil(n_steps / segs) steps each and the last segment what is left (where that leaves every segment a step).
inline void relay_schedule(int n_steps, int segs, double ratio, int* len) {   // len[segs]
  const int each = (n_steps + segs - 1) / segs;
  if (ratio >= 1.0 && n_steps - (segs - 1) * each >= 1) {
    for (int s = 0; s < segs; ++s) len[s] = s + 1 < segs ? each : n_steps - (segs - 1) * each;
    return;
  }
  if (ratio > 1.0) ratio = 1.0;
  double w = 1.0, sum = 0.0;
  for (int s = 0; s < segs; ++s) { sum += w; w *= ratio; }
  const int spare = n_steps - segs;
  int left = spare;
  w = 1.0;
  for (int s = 0; s < segs; ++s) {
    int extra = (int)((double)spare * (w / sum));
    if (extra > left) extra = left;
    len[s] = 1 + extra;
    left -= extra;
    w *= ratio;
  }
  for (int s = 0; left > 0; s = s + 1 < segs ? s + 1 : 0, --left) len[s] += 1;
}
// ratio of the library's own cut, in percent: chosen by measurement (profiles/r07_relay_schedule.txt)
constexpr int kSegRatioPct = 70;
// how a launch is cut: the ratio in percent, or explicit lengths (n_lens > 0: they sum to the launch's n_steps)
struct RelayCut { int ratio_pct = kSegRatioPct; int n_lens = 0; int lens[kSegTable] = {}; };
constexpr int kSegsDecide = 0;                                // RelayAsk::segs: the launcher decides with its kernel's occupancy
constexpr unsigned long long kSegTimeout = 6000000000ull;     // a minute of the 100 MHz clock
// The hand-over's form where nothing else is asked (kernels.h: relay_begin / relay_end have the forms): chosen by measurement,
// a form is taken only where every run with it was shorter than every run without (profiles/r08_relay_handover.txt).  The
// write-through publish is (headline launch - 1.1 %); one acquire per workgroup did not separate and stays behind its switch.
constexpr int kRelayMode = kRelayThrough;
// What an entry point hands a chain launcher beside the kernel's parameters.  As constructed it asks for no relay.
struct RelayAsk {
  int cus = 0;                    // CUs of the handle's device (relay decisions are made for it, not for the current one)
  int segs = 1;                   // kSegsDecide, a forced count (experiments), or 1: the launch stays whole
  RelayCut cut;
  // this launch's allocation, zeroed: a flag word for each of `blocks` chain blocks, then its ticket counter and failure word
  unsigned* flags = nullptr; int blocks = 0;
  unsigned* err_host = nullptr;   // the handle's pinned word a timed-out hand-over is reported through (relay_failed)
  unsigned long long timeout = kSegTimeout; int fault = 0;     // (test hook: segments never raise their flag)
  int mode = kRelayMode;          // the hand-over's form (kernels.h: kRelayThrough | kRelayGroup)
#ifdef ARP_EXP_RELAY_STAMPS
  unsigned long long* stamps = nullptr;
#endif
};
// no relay: the launch's steps in one segment (P.n_steps is set)
inline void relay_off(HmcParams& P) {
  P.segs = 1; P.seg_len = P.n_steps; P.seg_blocks = 0; P.seg_epoch = 0; P.seg_flags = nullptr;
  P.seg_ctrl = nullptr; P.seg_err_host = nullptr; P.seg_timeout = kSegTimeout; P.seg_fault = 0; P.seg_mode = 0;
  for (int& v : P.seg_start) v = 0;
#ifdef ARP_EXP_RELAY_STAMPS
  P.seg_stamps = nullptr;
#endif
}
// The launcher's decision for `kernel` over `blocks` chain blocks, written into P (which arrives with no relay).  Left to it,
// segments pay where the blocks are at least one round of resident workgroups: 8 from 512 steps per launch on, 4 from 256.
template <class F>
inline RelayGeometry relay_plan(HmcParams& P, const RelayAsk& ask, int blocks, F kernel) {
  int segs = ask.segs, occ = 0;       // occ: workgroups of `kernel` one CU holds, where that has to be asked
  if (segs == kSegsDecide) {
    static std::mutex mu;
    static std::map<const void*, int> occ_of;
    {
      std::lock_guard<std::mutex> lock(mu);
      auto it = occ_of.find((const void*)kernel);
      if (it == occ_of.end()) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kBlock, 0) != hipSuccess) occ = 0;
        occ_of[(const void*)kernel] = occ;
      } else {
        occ = it->second;
      }
    }
    const long long slots = (long long)occ * ask.cus;
    segs = (slots > 0 && blocks >= slots) ? (P.n_steps >= 512 ? 8 : (P.n_steps >= 256 ? 4 : 1)) : 1;
    // one workgroup per CU (German credit and time_series at 4 lanes per chain: 100 - 155 KB of LDS): a workgroup that waits for
    // its block holds the whole CU, and every hand-over invalidates the XCD's L2 under the tile stream -- measured + 0.1 % and
    // + 4.2 % (tools/experiments/relay_ab.py), so these launches stay whole
    if (occ < 2) segs = 1;
  }
  if (segs < 1 || !ask.flags || blocks > ask.blocks) segs = 1;
  if (segs > 1) {
    P.segs = segs; P.seg_len = (P.n_steps + segs - 1) / segs; P.seg_blocks = blocks; P.seg_epoch = 0u; P.seg_flags = ask.flags;
    P.seg_ctrl = ask.flags + ask.blocks; P.seg_err_host = ask.err_host; P.seg_timeout = ask.timeout; P.seg_fault = ask.fault;
    P.seg_mode = ask.mode;
#ifdef ARP_EXP_RELAY_STAMPS
    P.seg_stamps = ask.stamps;
#endif
    if (segs <= kSegTable) {
      int len[kSegTable];
      relay_schedule(P.n_steps, segs, ask.cut.ratio_pct / 100.0, len);
      P.seg_start[0] = 0;
      for (int i = 0; i < segs; ++i) P.seg_start[i + 1] = P.seg_start[i] + (ask.cut.n_lens == segs ? ask.cut.lens[i] : len[i]);
    }
  }
  return {{segs, blocks, occ}};
}
// `kernel` over `blocks` chain blocks x the segments relay_plan decides for it: its own arguments, then P with the decision
template <class F, class... Args>
inline RelayGeometry relay_launch(F kernel, int blocks, const HmcParams& P, const RelayAsk& ask, hipStream_t s, const Args&... args) {
  HmcParams Q = P;
  const RelayGeometry g = relay_plan(Q, ask, blocks, kernel);
  hipLaunchKernelGGL(kernel, dim3(blocks * Q.segs), dim3(kBlock), 0, s, args..., Q);
  return g;
}
// ARP_SEGMENT_LENS: explicit segment lengths of a launch of n_steps; a list that is not one is refused, never replaced
inline int relay_explicit_cut(const char* list, int n_steps, RelayCut* cut) {
  long long sum = 0; int n = 0;
  for (const char* p = list; *p;) {
    char* end = nullptr;
    const long v = strtol(p, &end, 10);
    if (end == p || (*end && *end != ',') || v < 1 || v > 0x7fffffff || n == kSegTable) {      // (no launch is longer than an int)
      set_error("ARP_SEGMENT_LENS: want 1 to " + std::to_string(kSegTable) + " comma-separated lengths >= 1, got '" + list + "'");
      return 1;
    }
    sum += cut->lens[n++] = (int)v;
    p = *end ? end + 1 : end;
  }
  if (sum != n_steps) {
    set_error("ARP_SEGMENT_LENS: the lengths '" + std::string(list) + "' sum to " + std::to_string(sum) + ", the launch has " +
              std::to_string(n_steps) + " steps");
    return 1;
  }
  cut->n_lens = n;
  return 0;
}
// ARP_RELAY_PUBLISH=fence|through, ARP_RELAY_ACQUIRE=wave|group: `name` set to `off` clears `bit` of *mode, to `on` sets it;
// anything else is refused, never replaced
inline int relay_mode_switch(const char* name, const char* off, const char* on, int bit, int* mode) {
  const char* e = debug_switch(name);
  if (!e) return 0;
  if (std::string(e) == on) { *mode |= bit; return 0; }
  if (std::string(e) == off) { *mode &= ~bit; return 0; }
  set_error(std::string(name) + ": want '" + off + "' or '" + on + "', got '" + e + "'");
  return 1;
}
// The ask of one launch of cfg's chains at K lanes per chain on a handle's device (`cus`, `err_host`: arp_model).  Where the
// launch cannot be cut -- `allowed` false, a short launch, few blocks -- *ask stays what RelayAsk() is and nothing is allocated.
inline int relay_prepare(int cus, unsigned* err_host, const arp_hmc_config* cfg, int K, bool allowed, hipStream_t stream,
                         RelayAsk* ask) {
  *ask = RelayAsk(); ask->cus = cus;
  // the hand-over's form (A/B and tests): a value that is none is refused on every chain launch, cut or not
  int mode = kRelayMode;
  if (relay_mode_switch("ARP_RELAY_PUBLISH", "fence", "through", kRelayThrough, &mode) ||
      relay_mode_switch("ARP_RELAY_ACQUIRE", "wave", "group", kRelayGroup, &mode)) return 1;
  if (!allowed) return 0;
  int segs = kSegsDecide, dbg = 0;
  RelayCut cut;
  // explicit lengths cut a launch of any length (the hand-over tests' short launches); everything else starts at 256 steps
  const char* lens = debug_switch("ARP_SEGMENT_LENS");
  if (!lens && cfg->n_steps < 256) return 0;
  if (debug_int("ARP_SEGMENTS", &dbg) && dbg >= 1 && dbg <= 64) segs = dbg;
  if (debug_int("ARP_SEGMENT_RATIO", &dbg) && dbg >= 1 && dbg <= 100) cut.ratio_pct = dbg;
  if (lens) {
    if (relay_explicit_cut(lens, cfg->n_steps, &cut)) return 1;
    segs = cut.n_lens;
  }
  if (segs == 1) return 0;
  const long long blocks = ((long long)cfg->n_chains * K + kBlock - 1) / kBlock;
  // no kernel gets segments below one round of two workgroups per CU (relay_plan): spare those launches the allocation
  if (segs == kSegsDecide && blocks < 2LL * cus) return 0;
  // one zeroed flag word per chain block, then the launch's ticket counter and its failure word
  void* flags = nullptr;
  size_t bytes = ((size_t)blocks + 2) * sizeof(unsigned);
#ifdef ARP_EXP_RELAY_STAMPS              // timing experiment only: kStamps words per workgroup behind the flags (kernels.h: relay_stamp)
  const size_t stamps_at = (bytes + 7) / 8 * 8;
  const int stamp_segs = segs > 0 ? segs : 8;
  bytes = stamps_at + (size_t)stamp_segs * blocks * kStamps * sizeof(unsigned long long);
#endif
  ARP_HIP_OK(hipMallocAsync(&flags, bytes, stream));
  const hipError_t zeroed = hipMemsetAsync(flags, 0, bytes, stream);
  if (zeroed != hipSuccess) {
    (void)hipFreeAsync(flags, stream);
    ARP_HIP_OK(zeroed);
  }
  ask->mode = mode;
  ask->segs = segs; ask->cut = cut; ask->flags = (unsigned*)flags; ask->blocks = (int)blocks; ask->err_host = err_host;
#ifdef ARP_EXP_RELAY_STAMPS
  ask->stamps = (unsigned long long*)((char*)flags + stamps_at);
#endif
  // test hooks (ARP_DEBUG=1 only): a short time-out, and segments that never raise their flag -- the failure path on demand
  if (debug_int("ARP_RELAY_TIMEOUT_MS", &dbg) && dbg > 0) ask->timeout = 100000ull * (unsigned long long)dbg;
  if (debug_int("ARP_RELAY_FAULT", &dbg) && dbg == 1) ask->fault = 1;
  return 0;
}
// `relay_err`: a handle's pinned word.  A relay launch of that handle had a hand-over time out since the last look: report it once
inline int relay_failed(unsigned* relay_err, const char* where) {
  if (!relay_err || __atomic_load_n(relay_err, __ATOMIC_ACQUIRE) == 0u) return 0;
  __atomic_store_n(relay_err, 0u, __ATOMIC_RELEASE);
  set_error(std::string(where) + ": a relay hand-over inside an earlier chain launch of this handle timed out (was the device "
            "taken away for a minute?); that launch left its chains partly advanced -- discard them");
  return 1;
}
// behind the launch that `ask` went to and that did `g`: its flags back to the stream's pool, then the launch's own status
inline int relay_release(const RelayAsk& ask, const RelayGeometry& g, hipError_t launched, hipStream_t stream) {
#ifdef ARP_EXP_RELAY_STAMPS
  // the launch's stamps into the file ARP_RELAY_STAMPS_OUT names (each launch overwrites it): segments, chain blocks, kStamps,
  // then kStamps 64-bit words per ticket -- tools/relay_stamps.py reads it.  Waits for the launch: an experiment build only.
  const char* out = ask.flags ? debug_switch("ARP_RELAY_STAMPS_OUT") : nullptr;
  if (out && g.v[0] > 1) {
    std::vector<unsigned long long> w(3 + (size_t)g.v[0] * g.v[1] * kStamps);
    w[0] = (unsigned long long)g.v[0]; w[1] = (unsigned long long)g.v[1]; w[2] = kStamps;
    ARP_HIP_OK(hipStreamSynchronize(stream));
    ARP_HIP_OK(hipMemcpy(w.data() + 3, ask.stamps, (w.size() - 3) * sizeof(w[0]), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(out, "wb")) {
      fwrite(w.data(), sizeof(w[0]), w.size(), f);
      fclose(f);
    }
  }
#endif
  if (ask.flags) ARP_HIP_OK(hipFreeAsync(ask.flags, stream));
  ARP_HIP_OK(launched);
  return 0;
}

}  // namespace arp
