// Stand-alone driver of d3dp_amd/csrc/ctx_plan.h and train_plan.h for tests/test_train_rows_host.py, after
// tests/train_attn_passes_driver.cpp: no HIP, no library.  It reads one case per line of stdin, tab-separated: mode channels heads
// hidden frames joints depth batch [NAME=value ...]; the switches go through the process environment and CtxEnv::from_process().
// One line per case on stdout, tab-separated: the return code, the message, the members of the context's plan D3DP_TRAIN_ROWS bears on
// as name=value -- train_rows_hi, the new one, first -- and, for a TRAIN context that plans, the step's rows_hi (plan_train_step on
// 256 CUs) and every offset and the total of train_layout as one `layout=` field.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../d3dp_amd/csrc/train_plan.h"

static std::string g_err;

int d3dp_fail(int code, const char* fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<std::string> f;
    std::stringstream ss(line);
    for (std::string tok; std::getline(ss, tok, '\t');) f.push_back(tok);
    if (f.size() < 8) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    d3dp_cfg g{};
    g.mode = std::stoi(f[0]); g.channels = std::stoi(f[1]); g.heads = std::stoi(f[2]); g.hidden = std::stoi(f[3]);
    g.frames = std::stoi(f[4]); g.joints = std::stoi(f[5]); g.depth = std::stoi(f[6]);
    const int B = std::stoi(f[7]);
    std::vector<std::string> names;
    for (size_t i = 8; i < f.size(); ++i) {
      const size_t eq = f[i].find('=');
      if (eq == std::string::npos) { fprintf(stderr, "bad switch: %s\n", f[i].c_str()); return 2; }
      names.push_back(f[i].substr(0, eq));
      setenv(names.back().c_str(), f[i].c_str() + eq + 1, 1);
    }
    g_err.clear();
    CtxPlan p;
    const int rc = plan_context(g, CtxEnv::from_process(), false, &p);
    for (const std::string& n : names) unsetenv(n.c_str());
    printf("%d\t%s\ttrain_rows_hi=%d\ttrain_passes=%d\ttrain_attn_passes=%d\ttrain_x2=%d\ttrain_attn_x2=%d\ttrain_long_attn=%d\t"
           "train_overlap=%d\ttrain_overlap_sets=%d",
           rc, g_err.c_str(), p.train_rows_hi, p.train_passes, p.train_attn_passes, p.train_x2, p.train_attn_x2, p.train_long_attn,
           p.train_overlap, p.train_overlap_sets);
    if (rc == D3DP_OK && g.mode == D3DP_MODE_TRAIN) {
      const TrainPlan P = plan_train_step(p, g, B, 256);
      const TrainLayout L = train_layout(g, B);
      printf("\trows_hi=%d\tpasses=%d\tmerged=%d\tln_direct=%d\tbatched=%d\tall_tn=%d\tlayout=", P.rows_hi, P.passes, P.merged, P.ln_direct,
             P.batched, P.lin[0].tn && P.lin[1].tn && P.lin[2].tn && P.lin[3].tn);
      const size_t offs[] = {L.temb, L.x_final, L.saved0, L.saved_stride, L.xn, L.y, L.hid, L.dA, L.dB, L.dC, L.dqkv, L.dh, L.z, L.At, L.Xt,
                             L.Wt, L.dtemb, L.stats, L.op_a, L.op_w, L.op_at, L.part, L.part_rem, L.slots, L.dy_set_floats, L.op_a2,
                             L.op_at2, L.part2, L.x_cols, L.x_block, L.w_rows, L.w_cols, L.w_block, L.Tp_max, L.stats_x2, L.red,
                             L.red_floats, L.total_floats};
      for (size_t o : offs) printf("%zu,", o);
    }
    printf("\n");
  }
  return 0;
}
