// Stand-alone driver of d3dp_amd/csrc/ctx_plan.h and train_plan.h for tests/test_train_attn_passes_host.py, after
// tests/train_long_driver.cpp: no HIP, no library.  Run without an argument it reads one case per line of stdin, tab-separated: mode
// channels heads hidden frames joints variants_built [NAME=value ...]; the switches go through the process environment and
// CtxEnv::from_process().  One line per case on stdout, tab-separated: the return code, the message, and the members
// D3DP_TRAIN_ATTN_PASSES bears on as name=value -- train_attn_passes, the new one, first.  Run with the argument `step` the same
// input gives, for the contexts that plan, the members of the training step's plan (plan_train_step, batch 2 on 256 CUs) instead:
// attn_passes, the new one, first.
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
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int main(int argc, char** argv) {
  const bool step = argc > 1 && !strcmp(argv[1], "step");
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<std::string> f;
    std::stringstream ss(line);
    for (std::string tok; std::getline(ss, tok, '\t');) f.push_back(tok);
    if (f.size() < 7) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    d3dp_cfg g{};
    g.mode = std::stoi(f[0]); g.channels = std::stoi(f[1]); g.heads = std::stoi(f[2]); g.hidden = std::stoi(f[3]);
    g.frames = std::stoi(f[4]); g.joints = std::stoi(f[5]); g.depth = 1;
    std::vector<std::string> names;
    for (size_t i = 7; i < f.size(); ++i) {
      const size_t eq = f[i].find('=');
      if (eq == std::string::npos) { fprintf(stderr, "bad switch: %s\n", f[i].c_str()); return 2; }
      names.push_back(f[i].substr(0, eq));
      setenv(names.back().c_str(), f[i].c_str() + eq + 1, 1);
    }
    g_err.clear();
    CtxPlan p;
    const int rc = plan_context(g, CtxEnv::from_process(), f[6] == "1", &p);
    for (const std::string& n : names) unsetenv(n.c_str());
    if (!step) {
      printf("%d\t%s\ttrain_attn_passes=%d\ttrain_passes=%d\ttrain_x2=%d\ttrain_attn_x2=%d\ttrain_long_attn=%d\ttrain_overlap=%d\t"
             "train_overlap_sets=%d\texact_impl_req=%d\thdp=%d\n",
             rc, g_err.c_str(), p.train_attn_passes, p.train_passes, p.train_x2, p.train_attn_x2, p.train_long_attn, p.train_overlap,
             p.train_overlap_sets, p.exact_impl_req, p.hdp);
      continue;
    }
    printf("%d\t%s", rc, g_err.c_str());
    if (rc == D3DP_OK && g.mode == D3DP_MODE_TRAIN) {
      const TrainPlan P = plan_train_step(p, g, 2, 256);
      printf("\tattn_passes=%d\tpasses=%d\tuse_x2=%d\tattn_x2_s=%d\tattn_x2_t=%d\tatt_direct_s=%d\tatt_direct_t=%d\tattn_bwd_chunked=%d\t"
             "overlap_sets=%d",
             P.attn_passes, P.passes, P.use_x2, P.path.attn_x2(0), P.path.attn_x2(1), P.att_direct(0), P.att_direct(1), P.attn_bwd_chunked,
             P.overlap_sets);
    }
    printf("\n");
  }
  return 0;
}
