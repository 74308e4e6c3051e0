// The adaptive quantisation rule (av1-base_amd/csrc/aq_rule.h) compiled for the host: tests/test_aq_host.py checks it against the numpy
// restatement (tests/aq_ref.py).
#include "../../av1-base_amd/csrc/aq_rule.h"

extern "C" int aq_log2_q4(unsigned x) { return av1mi_aq_log2_q4(x); }
extern "C" int aq_unit_energy(unsigned S, unsigned Q, int bit_depth) { return av1mi_aq_unit_energy(S, Q, bit_depth); }
// step 3: E of a superblock from its n units' e
extern "C" int aq_sb_energy(const int *e, int n) {
  unsigned sum = 0;
  for (int i = 0; i < n; i++) sum += (unsigned)e[i];
  return av1mi_aq_mean(sum, (unsigned)n);
}
// steps 4-6: the quantiser indices of a frame's N superblocks from their E; returns M
extern "C" int aq_frame_qindex(const int *E, int N, int strength, int base, int *qindex) {
  unsigned sum = 0;
  for (int i = 0; i < N; i++) sum += (unsigned)E[i];
  const int M = av1mi_aq_mean(sum, (unsigned)N);
  for (int i = 0; i < N; i++) qindex[i] = av1mi_aq_qindex_of(strength, E[i], M, base);
  return M;
}
