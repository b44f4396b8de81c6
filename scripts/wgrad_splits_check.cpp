// Does the one wgrad_pick_splits of ptlflow_amd/csrc/pfk_wgrad_reduce.h give, for every (tiles, M), what the two bodies it replaced
// gave?  Those bodies (pfk_wgrad.hip: K-steps of 32 pixels, >= 16 per slice; pfk_wgrad_b16.hip: K-steps of 64 pixels, the last one
// partial, >= 8 per slice, the debug knob, the `s > ksteps` clamp) are restated below as they stood.  Host only:
//   g++ -std=c++17 -O2 scripts/wgrad_splits_check.cpp -o wgrad_splits_check && ./wgrad_splits_check
// tiles 1..2048 x M in {1..70000 step 7} u {2^k - 1, 2^k, 2^k + 1 : k <= 40} x knob {0, 1, 3, 64, 100} (bf16 only).
#include <cstdio>
#include <vector>

static int wgrad_pick_splits(long long tiles, long long ksteps, int min_steps, int forced = 0) {      // as in pfk_wgrad_reduce.h
  long long s = forced;
  if (forced <= 0) {
    s = 1024 / (tiles > 0 ? tiles : 1);
    const long long max_s = ksteps / min_steps > 0 ? ksteps / min_steps : 1;
    if (s > max_s) s = max_s;
  }
  if (s > ksteps) s = ksteps;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

static int old_f32(long long tiles, long long M, long long target = 1024) {
  long long s = target / (tiles > 0 ? tiles : 1);
  const long long max_s = M / 512 > 0 ? M / 512 : 1;
  if (s > max_s) s = max_s;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

static int old_b16(long long tiles, long long M, int knob) {
  const int KS = 64;
  const long long ksteps = (M + KS - 1) / KS;
  long long s;
  if (knob > 0) {
    s = knob;
  } else {
    s = 1024 / (tiles > 0 ? tiles : 1);
    const long long max_s = ksteps / 8 > 0 ? ksteps / 8 : 1;
    if (s > max_s) s = max_s;
  }
  if (s > ksteps) s = ksteps;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

int main() {
  std::vector<long long> Ms;
  for (long long m = 1; m <= 70000; m += 7) Ms.push_back(m);
  for (int k = 0; k <= 40; ++k)
    for (long long dm = -1; dm <= 1; ++dm)
      if ((1LL << k) + dm > 0) Ms.push_back((1LL << k) + dm);
  const int knobs[] = {0, 1, 3, 64, 100};
  long long n = 0, bad = 0;
  for (long long tiles = 1; tiles <= 2048; ++tiles)
    for (long long M : Ms) {
      ++n;
      if (wgrad_pick_splits(tiles, M / 32, 16) != old_f32(tiles, M)) ++bad;
      for (int knob : knobs)
        if (wgrad_pick_splits(tiles, (M + 63) / 64, 8, knob) != old_b16(tiles, M, knob)) ++bad;
    }
  printf("%lld (tiles, M) pairs, %lld mismatches\n", n, bad);
  return bad ? 1 : 0;
}
