// Stand-alone driver of the mask_eqn code generator (land_trendr_amd/csrc/lt_index.h
// codegen_body and lt_mask.h codegen: host code, string building with snprintf buffers) for a
// build with AddressSanitizer / UBSan, run as a plain program (tests/test_mask_eqn.py).
//
// usage: mask_codegen_check <file>; the file holds records of {int32 expect_ok, lt_index_prog}
// written by the test from MaskProgram.to_c(): the corpus, a 64-operation 16-band program and the
// malformed programs. Every accepted program must give a source that names its kernels, every
// rejected one an empty source with a message; each program also goes through the index code
// generator, which must reject every mask program.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>  // the handle types of the headers' structs; no HIP call is made

#include "../../include/lt_abi.h"
#include "../../land_trendr_amd/csrc/lt_index.h"
#include "../../land_trendr_amd/csrc/lt_mask.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <programs>\n", argv[0]);
    return 2;
  }
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) {
    perror(argv[1]);
    return 2;
  }
  int n_ok = 0, n_bad = 0;
  for (;;) {
    int32_t expect = 0;
    if (fread(&expect, sizeof expect, 1, fh) != 1) break;
    // on the heap, exactly sized: a read past the program's end is an ASan report
    std::vector<lt_index_prog> P(1);
    if (fread(P.data(), sizeof(lt_index_prog), 1, fh) != 1) {
      fprintf(stderr, "truncated record %d\n", n_ok + n_bad);
      return 2;
    }
    std::string err;
    const std::string src = lt_msk::codegen(P[0], err);
    if (expect) {
      if (src.empty() || src.find("lt_mask_kernel(") == std::string::npos ||
          src.find("lt_mask_kernel_v4(") == std::string::npos) {
        fprintf(stderr, "record %d: rejected (%s)\n", n_ok + n_bad, err.c_str());
        return 1;
      }
      n_ok++;
    } else {
      if (!src.empty() || err.empty()) {
        fprintf(stderr, "record %d: a malformed program was accepted\n", n_ok + n_bad);
        return 1;
      }
      n_bad++;
    }
    // a mask program is never an index program: its root is a boolean (a malformed one still
    // goes through that generator's checks)
    std::string ierr;
    P[0].out_type = P[0].band_type;
    if (!lt_idx::codegen(P[0], ierr).empty() && expect) {
      fprintf(stderr, "record %d: the index generator accepted a mask program\n", n_ok + n_bad);
      return 1;
    }
  }
  fclose(fh);
  printf("ok %d accepted, %d rejected\n", n_ok, n_bad);
  return 0;
}
