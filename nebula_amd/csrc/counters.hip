// counters.hip -- how a query's device counters reach the host, and its timing: the publish
// kernel and the host spin on its sequence word (fetch_counters, wait_host_word), the counted
// stream synchronisation (host_sync_at), the pooled timing events and their deferred resolution.
// Used by GO (traverse.hip and its units), shortest paths (paths.hip) and the C API (capi.cpp).
#include <chrono>
#include <cstdio>
#include <thread>

#include "engine.h"
#include "go_launch.h"

namespace nbg {

// Copies n device counters into coherent host memory, then the sequence word: each thread's
// store is made visible system-wide before thread 0 publishes the sequence number.
// One wave copies the words (a lane per word, loads in flight together), and lane 0 publishes
// the sequence with one system-scope release store: one system fence (an L2 write-back) instead
// of one per word.  A single wave, so the release's wait on the wave's outstanding stores covers
// every copy.  (One thread copying every word waited on each load in turn: ~10 us more.)
__global__ void k_publish(const unsigned long long* src, int n, unsigned long long* __restrict__ dst,
                          unsigned long long* seq_slot, unsigned long long seq, int shards) {
  // shards > 1: word i is the sum of its shards src[i + s * kShardStride] (block_add_sums).  All
  // loads of a lane (<= 4 words x kSumShards shards; n <= 256) are issued before any add: one
  // round trip (a per-word shard loop had made this launch 3.6 -> 8.0 us, r12d)
  // (agent-scope loads: the words were added by other launches' atomics; a plain load may be
  // served by a stale copy -- twice this round a count came back low)
  auto ld = [&](size_t k) { return __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  if (shards <= 1) {
    unsigned long long x[4];  // every load issued before the stores (n <= 256: 4 words a lane)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = int(threadIdx.x) + 64 * j;
      x[j] = i < n ? ld(size_t(i)) : 0ull;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = int(threadIdx.x) + 64 * j;
      if (i < n) dst[i] = x[j];
    }
  } else {
    unsigned long long x[4][kSumShards];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int s = 0; s < kSumShards; s++) {
        const int i = int(threadIdx.x) + 64 * j;
        x[j][s] = i < n && s < shards ? ld(size_t(s) * kShardStride + size_t(i)) : 0ull;
      }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = int(threadIdx.x) + 64 * j;
      unsigned long long v = 0;
#pragma unroll
      for (int s = 0; s < kSumShards; s++) v += x[j][s];
      if (i < n) dst[i] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(seq_slot, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the device counters d[0, n) into host h[0, n) once every launch before has finished: a
// one-thread-block kernel writes them and a sequence word to coherent host memory and the host
// spins on the word (a memcpy + hipStreamSynchronize round trip cost ~19 us, tools/launch_gap);
// past 2 s without it the stream is synchronised the ordinary way, which reports a fault
void fetch_counters(Ctx& c, const unsigned long long* d, int n, unsigned long long* h, hipEvent_t before,
                    int shards) {
  if (n > 256) throw Error(NBG_E_INVALID_ARG, "fetch_counters: at most 256 words");
  if (before) NBG_HIP(hipEventRecord(before, c.stream));
  const uint64_t seq = ++c.pub_seq;
  k_publish<<<1, 64, 0, c.stream>>>(d, n, h, c.host_seq, seq, std::max(shards, 1));
  NBG_HIP(hipGetLastError());
  if (c.opt("wait_trace", 0)) fprintf(stderr, "[nbg wait] rank %d: counter fetch of %d words\n", c.rank, n);
  wait_host_word(c, c.host_seq, seq);
}

// one host wait on a word the device publishes with a system-scope release (k_publish, the
// paths kernels' last-block publications)
void wait_host_word(Ctx& c, const unsigned long long* word, uint64_t seq) {
  c.timing.host_waits++;
  // pure spin for the first ~100 us (most waits: a hop of tens of us), then yield the core
  // between polls (a long hop, or several in-process LocalComm ranks waiting at once)
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; spin++) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return;
    __builtin_ia32_pause();
    if ((spin & 255u) == 255u) {
      const auto dt = std::chrono::steady_clock::now() - t0;
      if (dt > std::chrono::microseconds(100)) std::this_thread::yield();
      if (dt > std::chrono::seconds(2)) {
        NBG_HIP(hipStreamSynchronize(c.stream));  // a fault surfaces here
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return;
        throw Error(NBG_E_DEVICE, "counter publication lost");
      }
    }
  }
}

// the query's device time (ev[0] -> ev[1]) once it is asked for: go_run does not wait for ev[1]
void resolve_total(Ctx& c) {
  if (!c.total_pending) return;
  c.total_pending = false;
  float ms = 0;
  if (hipEventSynchronize(c.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess)
    c.timing.total_ms = ms;
}

// a host wait of the engine on the device (Timing::host_waits counts them; waits inside the
// transport are not the engine's)
void host_sync_at(Ctx& c, const char* file, int line) {
  c.timing.host_waits++;
  if (c.opt("wait_trace", 0)) fprintf(stderr, "[nbg wait] rank %d: stream sync at %s:%d\n", c.rank, file, line);
  NBG_HIP(hipStreamSynchronize(c.stream));
}

// an event recorded on the engine stream for deferred hop timing (kNoEvent: hop_timing off)
size_t timing_event(Ctx& c) {
  if (!c.hop_timing) return kNoEvent;
  if (c.tev_used == c.tev.size()) {
    hipEvent_t e;
    NBG_HIP(hipEventCreate(&e));
    c.tev.push_back(e);
  }
  NBG_HIP(hipEventRecord(c.tev[c.tev_used], c.stream));
  return c.tev_used++;
}

void timing_reset(Ctx& c) {
  c.tev_used = 0;
  c.tpend.clear();
}
// adds the deferred expansion times to expand_ms and their hops (after the query's last sync)
void timing_resolve(Ctx& c) {
  for (const auto& p : c.tpend) {
    float ms = 0;
    if (p.a == kNoEvent || p.b == kNoEvent) continue;
    if (hipEventSynchronize(c.tev[p.b]) == hipSuccess && hipEventElapsedTime(&ms, c.tev[p.a], c.tev[p.b]) == hipSuccess) {
      const bool in_hop = p.hop >= 0 && p.hop < c.timing.n_hops && p.hop < NBG_MAX_HOP_STATS;
      if (p.kind == 1) {  // a bottom-up hop's first pass
        if (in_hop) c.timing.hops[p.hop].kernel_ms += ms;
        continue;
      }
      if (p.kind == 2) {  // an exchange between ranks
        c.timing.comm_ms += ms;
        continue;
      }
      c.timing.expand_ms += ms;
      if (in_hop) {
        c.timing.hops[p.hop].ms += ms;
        if (c.timing.hops[p.hop].mode == 0) c.timing.hops[p.hop].kernel_ms += ms;  // k_expand is the hop
      }
    }
  }
  timing_reset(c);
}

}  // namespace nbg
