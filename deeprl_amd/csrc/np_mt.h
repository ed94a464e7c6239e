// numpy's legacy RandomState stream (MT19937) as the seed lanes draw from it, word for word: what np_mt.hip's kernel and its host
// twin share.  A lane's step, in the order of support.plan_actor_epsilon_greedy then replay.draw_uniform_indices:
//   per transition  randint(n_actions, size=1), then rand(1) < epsilon in float64;
//   if it learns    attempts of randint(0, size), each kept iff the ring holds its transition and the n_step behind it (np_mt_valid;
//                   n_step = 1: the transition and the next), until `batch` are kept.
// word:     y = key[pos++], tempered; pos == 624 regenerates the key first (the twist), never ahead of time.
// randint:  rng = n - 1; rng == 0 is 0 and takes NO word; else mask = the smallest 2^j - 1 >= rng and every attempt takes one word,
//           v = word & mask, accepted iff v <= rng.
// rand:     two words, a = w0 >> 5, b = w1 >> 6, (a * 2^26 + b) / 2^53.
// Every data-dependent loop is bounded by kNpMtBudget words per step: an attempt is made only while the step has taken at most
// kNpMtBudget words; a draw that gives up is 0 (inside n_actions, inside the ring) and the lane's err word gets kNpMtErrBudget.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NP_MT_HD __host__ __device__ __forceinline__
#else
#define NP_MT_HD inline
#endif

constexpr int kNpMtN = 624, kNpMtM = 397;
constexpr int kNpMtStateWords = 628;        // dra_np_mt_state: key[624] | pos | 3 words of padding (16-byte multiple)
constexpr int kNpMtBudget = 4096;           // words of one step after which no further attempt is made (64 windows)
constexpr int kNpMtErrBudget = 1 << 30;     // the err word's bit of a lane that ran out of budget (the kernels' own err is a count)
constexpr int kNpMtMaxK = 8;                // replay_act.h's kMaxK
constexpr int kNpMtMaxBatch = 256;          // the update kernels' kMaxB

NP_MT_HD uint32_t np_mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// new key[i] of the twist from key[i], key[i + 1 mod N] and key[i + M mod N] as they stand when the serial loop reaches i
NP_MT_HD uint32_t np_mt_twist(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

NP_MT_HD uint32_t np_mt_mask(uint32_t rng) {
  uint32_t m = rng;
  m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16;
  return m;
}

NP_MT_HD double np_mt_double(uint32_t w0, uint32_t w1) {
  return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0;
}

constexpr int kNpMtMaxNStep = 8;            // the update kernels' longest window (dqn_mlp.hip's kMaxNStep)

// UniformReplay.valid_index at history_length = 1 over an n-step window: the ring holds the transition and the n_step behind it,
// none of them across the write position
NP_MT_HD bool np_mt_valid(uint32_t i, int64_t ring_pos, int64_t ring_size, int64_t n_step) {
  const int64_t v = (int64_t)i;
  return v + n_step < ring_pos || (v >= ring_pos && v + n_step < ring_size);
}

// how many slots np_mt_valid accepts: 0 = the rejection loop could never end
NP_MT_HD int64_t np_mt_valid_count(int64_t ring_pos, int64_t ring_size, int64_t n_step) {
  const int64_t lo = ring_pos - n_step > 0 ? ring_pos - n_step : 0, hi = ring_size - n_step - ring_pos > 0 ? ring_size - n_step - ring_pos : 0;
  return lo + hi;
}

// n_step = 1: what the lanes of the 1-step entries run
NP_MT_HD bool np_mt_valid(uint32_t i, int64_t ring_pos, int64_t ring_size) { return np_mt_valid(i, ring_pos, ring_size, 1); }
NP_MT_HD int64_t np_mt_valid_count(int64_t ring_pos, int64_t ring_size) { return np_mt_valid_count(ring_pos, ring_size, 1); }
