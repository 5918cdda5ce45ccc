// plan_check FILE: parse a plan blob with ym_plan_parse (no ym_model_desc) and print "OK" (exit 0) or the error
// text (exit 1).  Host-only; tests/test_plan_format.py builds it with the sanitizers and feeds it mutated blobs.
#include <cstdio>
#include <fstream>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: plan_check BLOB\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  // an exact-size heap copy, so a read past the blob's end is a read past an allocation
  std::vector<char> blob((size_t)f.tellg());
  f.seekg(0);
  if (!f.read(blob.data(), (std::streamsize)blob.size())) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  Plan plan;
  std::string err;
  const int rc = ym_plan_parse(blob.data(), blob.size(), nullptr, plan, err);
  if (rc == YM_OK) {
    printf("OK\n");
    return 0;
  }
  printf("%s\n", err.c_str());
  return rc == YM_EBLOB && !err.empty() ? 1 : 2;
}
