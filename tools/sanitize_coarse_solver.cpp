// sanitize_coarse_solver.cpp -- the host logic of the coarsest-solver switch (host/amg_setup.cpp: coarse_solver_code,
// coarse_solver_choice; host/saena_c_api.cpp: saena_amg_set_coarse_solver) under AddressSanitizer and UBSan, as a stand-alone program
// against the CPU build of the host library -- no interpreter, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -Iinclude tools/sanitize_coarse_solver.cpp \
//       saena_amd/csrc/host/*.cpp -lpthread -lrt -ldl -o sanitize_coarse_solver && ./sanitize_coarse_solver
// Every name and every refusal of the setter, a null name, a null handle, and the environment's precedence over the setter's value
// with SAENA_COARSE_SOLVER unset, set to each name, empty, and set to something that is no name.  Prints "every check passed" and
// returns 0, or the number of failed checks.
#include "../include/saena_c.h"
#include "../saena_amd/csrc/host/amg_setup.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main() {
    int failed = 0;
    auto want = [&](bool ok, const char *what) { if (!ok) { printf("FAILED: %s\n", what); ++failed; } };
    using saena_host::coarse_solver_choice;
    using saena_host::coarse_solver_code;
    want(coarse_solver_code("direct") == 1 && coarse_solver_code("cg") == 0 && coarse_solver_code("device_cg") == 2, "the three names");
    want(coarse_solver_code(nullptr) == -1 && coarse_solver_code("") == -1 && coarse_solver_code("CG") == -1 && coarse_solver_code("device_cg ") == -1, "what is no name");
    unsetenv("SAENA_COARSE_SOLVER");
    for (int v = 0; v <= 2; ++v) want(coarse_solver_choice(v) == v, "no variable: the setter's value");
    const char *names[] = {"cg", "direct", "device_cg"};
    for (int e = 0; e < 3; ++e) {
        setenv("SAENA_COARSE_SOLVER", names[e], 1);
        for (int v = 0; v <= 2; ++v) want(coarse_solver_choice(v) == e, "the variable names a solver: it wins");
    }
    for (const char *junk : {"", "lu", "2"}) {
        setenv("SAENA_COARSE_SOLVER", junk, 1);
        for (int v = 0; v <= 2; ++v) want(coarse_solver_choice(v) == v, "the variable names nothing: the setter's value");
    }
    unsetenv("SAENA_COARSE_SOLVER");

    saena_amg_h *S = saena_amg_new();
    for (const char *n : names) want(saena_amg_set_coarse_solver(S, n) == 0, "the setter takes a name");
    want(saena_amg_set_coarse_solver(S, "lu") == -1 && std::strstr(saena_last_error(), "none of direct, cg, device_cg") != nullptr, "the setter refuses another name and says which exist");
    want(saena_amg_set_coarse_solver(S, nullptr) == -1 && saena_amg_set_coarse_solver(nullptr, "cg") == -1, "null arguments");
    saena_amg_free(S);
    if (failed) printf("%d checks failed\n", failed); else printf("every check passed\n");
    return failed;
}
