// Stand-alone driver of d3dp_amd/csrc/train_plan.h for tests/test_train_plan_host.py: no HIP, no library.  One case per line of
// stdin, tab-separated: channels heads hidden frames joints depth B n_cu variants_built [NAME=value ...] -- a D3DP_MODE_TRAIN context
// created under those switches (plan_context, through the process environment like d3dp_create) and one step of batch size B on
// a device of n_cu CUs.  One line per case on stdout, tab-separated: plan_context's return code, its message, then every TrainPlan
// field and every TrainLayout member as name=value (enums as their integer values, in the order of their declaration).
#include <cstdarg>
#include <cstdio>
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

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<std::string> f;
    std::stringstream ss(line);
    for (std::string tok; std::getline(ss, tok, '\t');) f.push_back(tok);
    if (f.size() < 9) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    d3dp_cfg g{};
    g.mode = D3DP_MODE_TRAIN; g.channels = std::stoi(f[0]); g.heads = std::stoi(f[1]); g.hidden = std::stoi(f[2]);
    g.frames = std::stoi(f[3]); g.joints = std::stoi(f[4]); g.depth = std::stoi(f[5]);
    const int B = std::stoi(f[6]), n_cu = std::stoi(f[7]);
    std::vector<std::string> names;
    for (size_t i = 9; i < f.size(); ++i) {
      const size_t eq = f[i].find('=');
      if (eq == std::string::npos) { fprintf(stderr, "bad switch: %s\n", f[i].c_str()); return 2; }
      names.push_back(f[i].substr(0, eq));
      setenv(names.back().c_str(), f[i].c_str() + eq + 1, 1);
    }
    g_err.clear();
    CtxPlan c;
    const int rc = plan_context(g, CtxEnv::from_process(), f[8] == "1", &c);
    for (const std::string& n : names) unsetenv(n.c_str());
    printf("%d\t%s", rc, g_err.c_str());
    if (rc != D3DP_OK) { printf("\n"); continue; }
    const TrainPlan P = plan_train_step(c, g, B, n_cu);
    const TrainPath path = plan_train_path(c, g);
    const TrainLayout L = train_layout(g, B);
#define I(name, v) printf("\t%s=%lld", name, (long long)(v))
    I("use_x2", P.use_x2); I("attn_x2_s", P.path.attn_x2(0)); I("attn_x2_t", P.path.attn_x2(1)); I("needs_aux", P.path.needs_aux);
    I("path_agrees", path.use_x2 == P.path.use_x2 && path.attn_x2_s == P.path.attn_x2_s && path.attn_x2_t == P.path.attn_x2_t &&
                         path.needs_aux == P.path.needs_aux);
    I("T", P.T); I("passes", P.passes); I("overlap_sets", P.overlap_sets);
    const char* lin[4] = {"qkv", "proj", "fc1", "fc2"};
    for (int j = 0; j < 4; ++j) {
      const TrainLinear& p = P.lin[j];
      const std::string n = std::string(lin[j]) + "_";
      I((n + "N").c_str(), p.N); I((n + "K").c_str(), p.K); I((n + "tn").c_str(), p.tn); I((n + "Z").c_str(), p.Z);
      I((n + "Tp").c_str(), p.Tp); I((n + "pad_rows").c_str(), p.pad_rows);
      I((n + "src0").c_str(), (int)P.source(0, j)); I((n + "src1").c_str(), (int)P.source(1, j)); I((n + "src2").c_str(), (int)P.source(2, j));
      I((n + "fwd_tail").c_str(), (int)p.fwd_tail.form); I((n + "fwd_tail_Z").c_str(), p.fwd_tail.Z);
      I((n + "dgrad_tail").c_str(), (int)p.dgrad_tail.form); I((n + "dgrad_tail_Z").c_str(), p.dgrad_tail.Z);
    }
    I("ln_fused", P.ln_fused); I("ln_direct", P.ln_direct); I("att_direct_s", P.att_direct(0)); I("att_direct_t", P.att_direct(1));
    I("attn_t_f32_mfma", P.attn_t_f32_mfma); I("gelu_operand", P.gelu_operand); I("gip", P.gip); I("mip1", P.mip1); I("mip2", P.mip2);
    I("batched", P.batched); I("merged", P.merged); I("mZ", P.mZ); I("mTp", P.mTp); I("rows_fit", P.rows_fit); I("parts_fit", P.parts_fit);
#define LF(m) I("L_" #m, L.m)
    LF(T); LF(Tpad); LF(C); LF(Hd); LF(unit); LF(temb); LF(x_final); LF(saved0); LF(saved_stride); LF(o_xin); LF(o_qkv); LF(o_att);
    LF(o_xmid); LF(o_hpre); LF(o_xout); LF(xn); LF(y); LF(hid); LF(dA); LF(dB); LF(dC); LF(dqkv); LF(dh); LF(z); LF(At); LF(Xt); LF(Wt);
    LF(dtemb); LF(stats); LF(op_a); LF(op_w); LF(op_at); LF(part); LF(op_a2); LF(op_at2); LF(part2); LF(part_rem); LF(slots); LF(x_cols);
    LF(w_rows); LF(w_cols); LF(stats_x2); LF(red); LF(total_floats);
    LF(dy_set_floats); LF(part_floats); LF(part_rem_floats); LF(x_block); LF(w_block); LF(Tp_max); LF(stats_x2_stride); LF(red_floats);
    I("slot_bwd0", kTrainBwdSlot0); I("slot_qkv0", kTrainQkvSlot0); I("slot_pmax0", kTrainPmaxSlot0); I("slots", kTrainSlots);
    LF(ln_rows); LF(bias_rows); LF(head_rows); LF(embed_bias_rows); LF(group_slices);
    printf("\n");
  }
  return 0;
}
