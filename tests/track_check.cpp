// track_check MODE < input: the host build of what the tracker kernel shares with the host (csrc/ym_track.h).
//
//   track_check assign   stdin: problems "NR NC LIMIT" followed by NR * NC costs (row-major).  For each, one line
//                        "K r0 c0 r1 c1 ..." — the K pairs of ym_assign on the weights min(cost - LIMIT, 0), rows
//                        ascending.  The work arrays are exact-size heap blocks of kTrackDim + 1 entries, so a
//                        sanitizer build faults on any index outside them.
//   track_check kalman   stdin: steps "I z0 z1 z2 z3" (initiate from a measurement), "P" (predict), "Z" (zero mean[7],
//                        as for a lost track), "U z0 z1 z2 z3" (update).  After each step one line: the 8 mean values,
//                        then the 64 covariance values, "%.17g".
//   track_check iou      stdin: pairs of boxes (8 floats per line); one fp32 IoU per line, "%.9g".
// Exit 0; 2 on a usage or input error.  Host-only; tests/test_track_host.py builds it with ASan / UBSan where the
// compiler has their runtimes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_track.h"

static int run_assign() {
  std::vector<double> u(kTrackDim + 1), v(kTrackDim + 1), minv(kTrackDim + 1);
  std::vector<int> p(kTrackDim + 1), way(kTrackDim + 1), sel(kTrackDim + 1);
  std::vector<unsigned char> used(kTrackDim + 1);
  const AssignWork ws{u.data(), v.data(), minv.data(), p.data(), way.data(), sel.data(), used.data()};
  int nr, nc;
  double limit;
  while (scanf("%d %d %lf", &nr, &nc, &limit) == 3) {
    if (nr < 0 || nc < 0 || nr > kTrackDim || nc > kTrackDim) return 2;
    std::vector<double> cost((size_t)nr * nc);
    for (double& c : cost)
      if (scanf("%lf", &c) != 1) return 2;
    std::vector<int> r2c(nr > 0 ? nr : 1, -2);
    const double* cp = cost.data();
    auto w = [cp, nc, limit](int i, int j) {
      const double c = cp[(size_t)i * nc + j];
      return c < limit ? c - limit : 0.0;
    };
    ym_assign(nr, nc, w, SerialLanes{}, ws, r2c.data());
    int k = 0;
    for (int i = 0; i < nr; ++i) k += r2c[i] >= 0;
    printf("%d", k);
    for (int i = 0; i < nr; ++i) {
      if (r2c[i] >= nc || r2c[i] < -1) return 2;
      if (r2c[i] >= 0) printf(" %d %d", i, r2c[i]);
    }
    printf("\n");
  }
  return 0;
}

static int run_kalman() {
  double mean[8] = {0}, cov[64] = {0}, z[4];
  char op[8];
  while (scanf("%7s", op) == 1) {
    if (op[0] == 'I' || op[0] == 'U') {
      if (scanf("%lf %lf %lf %lf", &z[0], &z[1], &z[2], &z[3]) != 4) return 2;
      if (op[0] == 'I') ym_kf_initiate(z, mean, cov);
      else ym_kf_update(mean, cov, z);
    } else if (op[0] == 'P') {
      ym_kf_predict(mean, cov);
    } else if (op[0] == 'Z') {
      mean[7] = 0;
    } else {
      return 2;
    }
    for (int i = 0; i < 8; ++i) printf("%.17g ", mean[i]);
    for (int i = 0; i < 64; ++i) printf("%.17g%c", cov[i], i == 63 ? '\n' : ' ');
  }
  return 0;
}

static int run_iou() {
  float b[8];
  while (scanf("%f %f %f %f %f %f %f %f", &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &b[7]) == 8)
    printf("%.9g\n", (double)ym_iou32(b, b + 4));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "assign")) return run_assign();
  if (argc == 2 && !strcmp(argv[1], "kalman")) return run_kalman();
  if (argc == 2 && !strcmp(argv[1], "iou")) return run_iou();
  fprintf(stderr, "usage: track_check assign|kalman|iou < input\n");
  return 2;
}
