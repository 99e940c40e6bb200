// Stand-alone driver of d3dp_amd/csrc/sampler_plan.h for tests/test_sampler_plan_host.py: no HIP, no library.
//   argv[1]: a file of T raw float64 values, the schedule's alphas_cumprod
//   argv[2], argv[3] (optional): the same for the module's sqrt_recip_alphas_cumprod / sqrt_recipm1_alphas_cumprod buffers
//   stdin:   one case per line, "K eta"
//   stdout:  one line per case: return code, message, then per step the fields as INTEGERS -- doubles as the int64 of their
//            bits, floats as the int32 of theirs -- "t:sqrt_recip:sqrt_recipm1:c_xstart:c_noise:sigma:last:c_noise64", tab-separated.
// A last case "check <K> <last flags...>" runs check_ddim_steps on a table with those flags instead.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../d3dp_amd/csrc/sampler_plan.h"

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

static long long bits64(double v) { long long b; memcpy(&b, &v, 8); return b; }
static int bits32(float v) { int b; memcpy(&b, &v, 4); return b; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  auto read = [](const char* path, std::vector<double>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    double v;
    while (fread(&v, 8, 1, f) == 1) out.push_back(v);
    fclose(f);
    return true;
  };
  std::vector<double> ac, sr, srm1;
  if (!read(argv[1], ac)) return 2;
  if (argc >= 4 && (!read(argv[2], sr) || !read(argv[3], srm1) || sr.size() != ac.size() || srm1.size() != ac.size())) return 2;
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    g_err.clear();
    if (!strncmp(line, "check", 5)) {
      std::vector<d3dp_ddim_step> steps;
      int K = 0, pos = 0, n = 0;
      sscanf(line + 5, "%d%n", &K, &pos);
      const char* p = line + 5 + pos;
      int flag;
      while (sscanf(p, "%d%n", &flag, &n) == 1) {
        d3dp_ddim_step s{};
        s.last = flag;
        steps.push_back(s);
        p += n;
      }
      const int rc = check_ddim_steps(steps.empty() ? nullptr : steps.data(), K);
      printf("%d\t%s\n", rc, g_err.c_str());
      continue;
    }
    int K = 0;
    double eta = 1.0;
    if (sscanf(line, "%d %lf", &K, &eta) != 2) return 3;
    std::vector<d3dp_ddim_step> steps((size_t)(K > 0 ? K : 1));
    const int rc = plan_ddim_steps(ac.data(), sr.empty() ? nullptr : sr.data(), srm1.empty() ? nullptr : srm1.data(), (int)ac.size(), K, eta,
                                   steps.data());
    printf("%d\t%s", rc, g_err.c_str());
    if (rc == 0)
      for (int k = 0; k < K; ++k) {
        const d3dp_ddim_step& s = steps[k];
        printf("\t%lld:%lld:%lld:%d:%d:%d:%d:%lld", (long long)s.t, bits64(s.sqrt_recip), bits64(s.sqrt_recipm1), bits32(s.c_xstart),
               bits32(s.c_noise), bits32(s.sigma), s.last, bits64(s.c_noise64));
      }
    printf("\n");
  }
  return 0;
}
