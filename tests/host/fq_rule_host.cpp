// The frame term of the quantiser (av1-base_amd/csrc/tpl_rule.h: av1mi_fq_*) compiled for the host: tests/test_fq_host.py checks it
// against the numpy restatement (tests/fq_ref.py).
#include "../../av1-base_amd/csrc/tpl_rule.h"

extern "C" int fq_beta(unsigned long long OF, unsigned long long PF) { return av1mi_fq_beta(OF, PF); }
extern "C" int fq_mean(unsigned long long sum, unsigned long long n) { return av1mi_fq_mean(sum, n); }
extern "C" int fq_step(int strength, int betaF, int MF, int base) { return av1mi_fq_step(strength, betaF, MF, base); }
extern "C" int fq_qindex(int strength, int betaF, int MF, int base) { return av1mi_fq_qindex(strength, betaF, MF, base); }
extern "C" int fq_sb_qindex(int aq, int E, int M, int tpl, int beta, int Mb_f, int q_f) { return av1mi_fq_sb_qindex(aq, E, M, tpl, beta, Mb_f, q_f); }
extern "C" int fq_min_step() { return AV1MI_FQ_MIN_STEP; }
extern "C" int fq_max_step() { return AV1MI_FQ_MAX_STEP; }
extern "C" int fq_max_strength() { return AV1MI_FQ_MAX_STRENGTH; }
