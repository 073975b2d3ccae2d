// sanitize_devmem.cpp -- the logic of saena_amd/csrc/devmem.h (the owner of the library's device and pinned arrays) under
// AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program on the host: DEVMEM_HOST_TEST puts malloc / free in the
// place of hipMalloc / hipFree, everything else is the header as the library compiles it.
//   g++ -std=c++17 -O1 -g -DDEVMEM_HOST_TEST -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/sanitize_devmem.cpp -o sanitize_devmem && ./sanitize_devmem
// (tests/test_devmem.py builds and runs exactly this).
// Move, self-move, reset, assignment from {}, the refusal of a second alloc, a group of owners freed by assignment, owners in a
// vector, and the arithmetic of the live-byte counter.  A leak or a double free is the sanitizer's to report (another exit
// status); a wrong count or pointer fails a check below.
#include "../saena_amd/csrc/devmem.h"

#include <cstdio>
#include <utility>
#include <vector>

using devmem::DevArr;
using devmem::PinArr;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static long long live() { return (long long)devmem::live_bytes.load(); }

struct Group { DevArr<double> val; DevArr<int> ptr; bool ok = false; char tried = 0; };

int main() {
    const long long base = live();
    {   // empty by default; alloc, bytes, conversion, writes inside the array
        DevArr<double> a;
        CHECK(!a && a.get() == nullptr && a.bytes() == 0);
        CHECK(a.alloc(100) == hipSuccess);
        CHECK(a && a.bytes() == 800 && live() == base + 800);
        double *p = a;
        for (int i = 0; i < 100; ++i) p[i] = i;
        CHECK((a + 99)[0] == 99.0);
        // a second alloc is refused and changes nothing
        CHECK(a.alloc(10) == hipErrorInvalidValue);
        CHECK(a.get() == p && a.bytes() == 800 && live() == base + 800);
        // reset frees, and the object can be used again
        a.reset();
        CHECK(!a && a.bytes() == 0 && live() == base);
        a.reset();
        CHECK(live() == base);
        CHECK(a.alloc(3) == hipSuccess && live() == base + 24);
        a = {};
        CHECK(!a && live() == base);
    }
    {   // move construction and move assignment hand the array over; the target's own array is freed
        DevArr<int> a, b;
        CHECK(a.alloc(8) == hipSuccess && b.alloc(2) == hipSuccess && live() == base + 40);
        int *pa = a;
        DevArr<int> c(std::move(a));
        CHECK(!a && c.get() == pa && c.bytes() == 32 && live() == base + 40);
        b = std::move(c);
        CHECK(!c && b.get() == pa && b.bytes() == 32 && live() == base + 32);
        DevArr<int> &self = b;
        b = std::move(self);                                       // self-move keeps the array
        CHECK(b.get() == pa && b.bytes() == 32 && live() == base + 32);
        CHECK(a.alloc(1) == hipSuccess && live() == base + 36);    // a moved-from object is empty and may allocate
    }
    CHECK(live() == base);                                         // destructors
    {   // a group of owners with its flags: assignment from {} frees the arrays and clears the flags
        Group g;
        CHECK(g.val.alloc(16) == hipSuccess && g.ptr.alloc(5) == hipSuccess);
        g.ok = true; g.tried = 1;
        CHECK(live() == base + 148);
        g = {};
        CHECK(!g.val && !g.ptr && !g.ok && g.tried == 0 && live() == base);
        Group two[2];
        CHECK(two[1].val.alloc(1) == hipSuccess);
        two[1] = {};
        CHECK(live() == base);
    }
    {   // owners in a vector (the per-level work vectors); pinned owners share the counter
        std::vector<DevArr<double>> v(4);
        for (size_t i = 0; i < v.size(); ++i) CHECK(v[i].alloc(i + 1) == hipSuccess);
        CHECK(live() == base + 80);
        v.erase(v.begin());
        CHECK(live() == base + 72 && v[0].bytes() == 16);
        PinArr<double> h;
        CHECK(h.alloc(2) == hipSuccess && live() == base + 88);
        v.clear();
        CHECK(live() == base + 16);
    }
    CHECK(live() == base);
    {   // an allocation of no bytes holds nothing the counter would see
        DevArr<char> z;
        CHECK(z.alloc(0) == hipSuccess && z.bytes() == 0);
        z.reset();
        CHECK(live() == base);
    }
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("ok");
    return 0;
}
