"""saena_amd/csrc/dispatch.h (among / with_bool: the runtime value -> compile-time constant step of every kernel picker in
sgpu_runtime.hip) as a stand-alone host program: the header has no HIP in it, so g++ -std=c++17 compiles and runs it here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "dispatch.h"
#include <cstdio>
#include <initializer_list>
#include <type_traits>
using dispatch::among;
using dispatch::with_bool;

static int calls = 0, bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

// stands for a kernel template: a distinct function per parameter set, picked as a pointer like a __global__ instantiation
using Fn = int (*)();
template <int A, int B, bool H> int kernel() { return A * 1000 + B * 10 + (H ? 1 : 0); }

static Fn pick(int a, int b, bool h) {
    return among<0, 2, 6>(a, [&](auto A) {
        return among<1, 4, 64>(b, [&](auto B) {
            return with_bool(h, [&](auto H) -> Fn { ++calls; return kernel<A(), B(), H()>; }); }); });
}

int main() {
    // every listed value reaches f with exactly that constant, f runs once; the list need not be sorted or start at zero
    for (int v : {7, -3, 0, 64, 2}) {
        calls = 0;
        const int got = among<7, -3, 0, 64, 2>(v, [&](auto V) {
            ++calls;
            static_assert(std::is_same<decltype(V), std::integral_constant<int, V()>>::value, "an integral_constant<int, Vk>");
            static_assert(V() == 7 || V() == -3 || V() == 0 || V() == 64 || V() == 2, "f is instantiated for listed values only");
            return 1000 + V(); });
        EXPECT(got == 1000 + v);
        EXPECT(calls == 1);
    }
    // a value that is not listed: f is not called, the result is value-initialised (0, nullptr) -- also for 0 itself, which the
    // result type is NOT deduced from (the static_assert above would fail to compile)
    for (int v : {1, 3, 63, 65, -1, 1 << 30}) {
        calls = 0;
        EXPECT((among<7, -3, 0, 64, 2>(v, [&](auto V) { ++calls; return 1000 + V(); }) == 0));
        EXPECT((among<7, 64>(v, [&](auto V) -> Fn { ++calls; return kernel<V(), 0, false>; }) == nullptr));
        EXPECT((among<7, 64>(v, [&](auto V) -> const char * { ++calls; return V() ? "k" : "0"; }) == nullptr));
        EXPECT(calls == 0);
    }
    calls = 0;
    EXPECT((among<5, 9>(0, [&](auto V) { static_assert(V() != 0, "not listed"); ++calls; return V() + 1; }) == 0));
    EXPECT(calls == 0);
    // a value listed twice still reaches f once
    calls = 0;
    EXPECT((among<4, 4, 8>(4, [&](auto V) { ++calls; return (int)V(); }) == 4));
    EXPECT(calls == 1);
    // with_bool: exactly std::true_type / std::false_type, once
    for (bool b : {false, true}) {
        calls = 0;
        const int got = with_bool(b, [&](auto B) {
            ++calls;
            static_assert(std::is_same<decltype(B), std::true_type>::value || std::is_same<decltype(B), std::false_type>::value, "a bool constant");
            return B() ? 11 : 22; });
        EXPECT(got == (b ? 11 : 22));
        EXPECT(calls == 1);
    }
    // three deep (among in among in with_bool): the innermost result comes back, f ran once; unlisted at either level: nullptr, no call
    for (int a : {0, 2, 6})
        for (int b : {1, 4, 64})
            for (bool h : {false, true}) {
                calls = 0;
                const Fn k = pick(a, b, h);
                EXPECT(k != nullptr && k() == a * 1000 + b * 10 + (h ? 1 : 0));
                EXPECT(calls == 1);
            }
    calls = 0;
    EXPECT(pick(1, 4, true) == nullptr);
    EXPECT(pick(2, 5, false) == nullptr);
    EXPECT(pick(7, 7, true) == nullptr);
    EXPECT(calls == 0);
    EXPECT(pick(2, 4, true) != pick(2, 4, false) && pick(2, 4, true) != pick(6, 4, true));
    if (bad) return 1;
    std::printf("ok\n");
    return 0;
}
"""


def test_among_and_with_bool(tmp_path):
    src, exe = str(tmp_path / "dispatch_check.cpp"), str(tmp_path / "dispatch_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "saena_amd", "csrc"), src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
