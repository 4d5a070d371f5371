// Stand-alone host check of the pruning and evaluation twins (csrc/ngram_prune.h), for a sanitizer build of HOST code only:
//   cd asr_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer -x hip api.cpp decode.hip ../../scripts/host_check_ngram_prune.cpp -o /tmp/host_check_ngram_prune
//   ASAN_OPTIONS=detect_leaks=0 /tmp/host_check_ngram_prune
// It needs no GPU: only the *_host entries are called.  The corpus is the suite's TINY (6 sentences over a, b, c) at order 3 and the
// threshold 5e-3 of tests/test_cpu_ngram_prune.py, whose restatement keeps 6 (<unk> among them), 10 and 5 n-grams.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "ds2hip.h"

typedef unsigned long long u64;

#define CHECK(call)                                                   \
  do {                                                                \
    if (call) {                                                       \
      fprintf(stderr, "%s failed: %s\n", #call, ds2_last_error());    \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  const int N = 3, n_vocab = 6;
  const std::vector<int> tokens = {3, 4, 5, 3, 4, 4, 5, 3, 5, 3, 3, 4, 4};
  const std::vector<long long> off = {0, 3, 5, 8, 9, 12, 13};
  const long long n_sent = (long long)off.size() - 1, n_tok = (long long)tokens.size();
  const double fallback[3] = {0.5, 1.0, 1.5};
  // the estimate
  const long long cap[3] = {64, 64, 64};
  std::vector<u64> keys[3];
  std::vector<unsigned> count[3], adj[3];
  std::vector<double> lp[3], lb[3];
  u64* kp[3];
  unsigned *cp[3], *ap[3];
  double *pp[3], *bp[3];
  for (int n = 0; n < N; ++n) {
    keys[n].resize(64), count[n].resize(64), adj[n].resize(64), lp[n].resize(64), lb[n].resize(64);
    kp[n] = keys[n].data(), cp[n] = count[n].data(), ap[n] = adj[n].data(), pp[n] = lp[n].data(), bp[n] = lb[n].data();
  }
  long long distinct[3], coc[12];
  double D[12], unk;
  int fell[3];
  CHECK(ds2_ngram_estimate_host(tokens.data(), n_tok, off.data(), n_sent, n_vocab, N, fallback, cap, kp, cp, ap, pp, bp, distinct, coc, D, fell,
                                &unk));
  // the model: exactly-sized arrays (so that a read past the end is seen), <unk> as row 0 of the 1-grams
  std::vector<u64> mk[3];
  std::vector<double> mp[3], mb[3];
  for (int n = 0; n < N; ++n) {
    if (n == 0) mk[0].push_back(0), mp[0].push_back(unk), mb[0].push_back(NAN);
    mk[n].insert(mk[n].end(), keys[n].begin(), keys[n].begin() + distinct[n]);
    mp[n].insert(mp[n].end(), lp[n].begin(), lp[n].begin() + distinct[n]);
    mb[n].insert(mb[n].end(), lb[n].begin(), lb[n].begin() + distinct[n]);
  }
  long long cnt[3];
  void *K[3], *P[3], *B[3];
  auto bind = [&]() {
    for (int n = 0; n < N; ++n) cnt[n] = (long long)mk[n].size(), K[n] = mk[n].data(), P[n] = mp[n].data(), B[n] = mb[n].data();
  };
  bind();
  // evaluation of the training text and of an empty sentence, an OOV (<unk>, id 0) among them
  const std::vector<int> held = {3, 4, 5, 0, 4, 5};
  const std::vector<long long> hoff = {0, 3, 3, 6};
  std::vector<double> out_lp(held.size() + 3);
  std::vector<int> out_order(held.size() + 3);
  CHECK(ds2_ngram_eval_host(held.data(), (long long)held.size(), hoff.data(), 3, n_vocab, N, cnt, K, P, B, out_lp.data(), out_order.data()));
  double total = 0.0;
  for (size_t i = 0; i < out_lp.size(); ++i) {
    if (out_order[i] < 1 || !(out_lp[i] < 0.0)) {
      fprintf(stderr, "position %zu: order %d log10 p %g\n", i, out_order[i], out_lp[i]);
      return 1;
    }
    total += out_lp[i];
  }
  // marking
  const double theta = 5e-3;
  std::vector<double> q[3], sp[3], sq[3], val[3];
  std::vector<unsigned char> mark[3];
  void *Q[3] = {}, *SP[3] = {}, *SQ[3] = {}, *V[3] = {}, *M[3] = {};
  for (int n = 2; n <= N; ++n) {
    q[n - 1].resize(cnt[n - 1]), val[n - 1].resize(cnt[n - 1]), mark[n - 1].resize(cnt[n - 1]);
    sp[n - 1].resize(cnt[n - 2]), sq[n - 1].resize(cnt[n - 2]);
    CHECK(ds2_ngram_prune_sums_host(n_vocab, N, cnt, K, P, B, n, q[n - 1].data(), sp[n - 1].data(), sq[n - 1].data()));
    Q[n - 1] = q[n - 1].data(), SP[n - 1] = sp[n - 1].data(), SQ[n - 1] = sq[n - 1].data(), V[n - 1] = val[n - 1].data(),
           M[n - 1] = mark[n - 1].data();
  }
  CHECK(ds2_ngram_prune_entropy_host(n_vocab, N, cnt, K, P, B, Q, SP, SQ, theta, V, M));
  for (int n = N; n >= 3; --n) CHECK(ds2_ngram_prune_closure_host(n_vocab, N, cnt, K, P, B, n, mark[n - 1].data(), mark[n - 2].data()));
  // the kept rows, then the new backoffs bottom up
  for (int n = 2; n <= N; ++n) {
    size_t w = 0;
    for (size_t r = 0; r < mk[n - 1].size(); ++r)
      if (!mark[n - 1][r]) mk[n - 1][w] = mk[n - 1][r], mp[n - 1][w] = mp[n - 1][r], mb[n - 1][w] = mb[n - 1][r], ++w;
    mk[n - 1].resize(w), mp[n - 1].resize(w), mb[n - 1].resize(w);
    mk[n - 1].shrink_to_fit(), mp[n - 1].shrink_to_fit(), mb[n - 1].shrink_to_fit();
  }
  bind();
  for (int n = 1; n < N; ++n) {
    std::vector<double> a(cnt[n - 1]), c(cnt[n - 1]);
    CHECK(ds2_ngram_prune_sums_host(n_vocab, N, cnt, K, P, B, n + 1, nullptr, a.data(), c.data()));
    CHECK(ds2_ngram_prune_backoff_host(cnt[n - 1], a.data(), c.data(), mb[n - 1].data()));
  }
  printf("log10 p of the held-out text %.12f; kept %lld %lld %lld\n", total, cnt[0], cnt[1], cnt[2]);
  if (cnt[0] != 6 || cnt[1] != 10 || cnt[2] != 5) {
    fprintf(stderr, "expected 6 10 5\n");
    return 1;
  }
  // a refusal goes through the error path as well
  if (!ds2_ngram_prune_entropy_host(n_vocab, N, cnt, K, P, B, Q, SP, SQ, 0.0, V, M)) return 1;
  return 0;
}
