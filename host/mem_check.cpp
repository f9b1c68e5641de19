// mem_check.cpp -- the owner of libsdrx's device and pinned memory (sdrreceiver_amd/csrc/sdrx_mem.h) over a fake memory policy:
// counting malloc / free that records the live blocks and fails the k-th allocation on request.  Walks what no GPU test can
// reach -- allocations that fail -- next to the ordinary life of a buffer; exits non-zero on any violation.  Plain C++17, no HIP:
//   g++ -std=c++17 -fsanitize=address,undefined host/mem_check.cpp && ./a.out     (tests/test_device_memory_host.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "../sdrreceiver_amd/csrc/sdrx_mem.h"

namespace {

struct Fake {
    using error = int;
    static constexpr error ok = 0;
    static std::set<void *> live;
    static int obtained, released, cleared, double_release;
    static int fail_at; // the fail_at-th obtain from now on fails (1: the next one); 0: none
    static error obtain(void **p, size_t bytes)
    {
        if (fail_at > 0 && --fail_at == 0)
            return 2; // (as hipErrorOutOfMemory)
        *p = malloc(bytes ? bytes : 1);
        memset(*p, 0xA5, bytes);
        live.insert(*p);
        ++obtained;
        return ok;
    }
    static error clear(void *p, size_t bytes)
    {
        memset(p, 0, bytes);
        ++cleared;
        return ok;
    }
    static void release(void *p)
    {
        if (!live.erase(p)) {
            ++double_release;
            return;
        }
        ++released;
        free(p);
    }
};
std::set<void *> Fake::live;
int Fake::obtained = 0, Fake::released = 0, Fake::cleared = 0, Fake::double_release = 0, Fake::fail_at = 0;

template <class T>
using Buf = sdrx::Owned<T, Fake>;

int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "mem_check: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

template <class T>
bool empty(const Buf<T> &b)
{
    return b.get() == nullptr && b.count() == 0 && b.bytes() == 0 && !b;
}

void life_of_a_buffer()
{
    Buf<double> a;
    CHECK(empty(a));
    CHECK(a.alloc(100, true) == Fake::ok);
    CHECK(a.get() && a.count() == 100 && a.bytes() == 800 && Fake::live.size() == 1 && Fake::cleared == 1);
    bool zero = true;
    for (int i = 0; i < 100; ++i)
        zero = zero && a[i] == 0.0; // (the implicit conversion to a raw pointer)
    CHECK(zero);
    double *was = a;
    Buf<double> b(std::move(a)); // move construction: ownership travels, nothing is obtained or released
    CHECK(empty(a) && b.get() == was && b.count() == 100 && Fake::live.size() == 1);
    Buf<double> c;
    CHECK(c.alloc(7) == Fake::ok && Fake::live.size() == 2 && Fake::cleared == 1);
    c = std::move(b); // move assignment: what c held is released
    CHECK(empty(b) && c.get() == was && c.bytes() == 800 && Fake::live.size() == 1 && Fake::released == 1);
    Buf<double> &same = c;
    c = std::move(same); // (self-assignment keeps it)
    CHECK(c.get() == was && Fake::live.size() == 1);
    CHECK(c.alloc(3) == Fake::ok && c.count() == 3 && Fake::live.size() == 1 && Fake::released == 2); // alloc replaces
    c.reset();
    CHECK(empty(c) && Fake::live.empty());
    c.reset(); // (twice is once)
    CHECK(Fake::double_release == 0);
    {
        Buf<int> d;
        CHECK(d.alloc(5) == Fake::ok && Fake::live.size() == 1);
    } // destruction
    CHECK(Fake::live.empty() && Fake::obtained == Fake::released);
    Buf<int> e;
    CHECK(e.alloc(4) == Fake::ok);
    Fake::fail_at = 1; // a failed alloc leaves the owner empty -- and has released what it held
    CHECK(e.alloc(8) != Fake::ok && empty(e) && Fake::live.empty() && Fake::fail_at == 0);
}

void reserve_grows_only()
{
    const int obtained = Fake::obtained, released = Fake::released;
    Buf<float> a;
    CHECK(a.reserve(0) == Fake::ok && empty(a) && Fake::obtained == obtained);
    CHECK(a.reserve(64) == Fake::ok && a.count() == 64 && Fake::obtained == obtained + 1);
    float *was = a;
    CHECK(a.reserve(64) == Fake::ok && a.reserve(10) == Fake::ok); // below and at capacity: nothing happens
    CHECK(a.get() == was && a.count() == 64 && Fake::obtained == obtained + 1 && Fake::released == released);
    CHECK(a.reserve(65) == Fake::ok && a.count() == 65 && a.bytes() == 260); // above: released, then obtained
    CHECK(Fake::obtained == obtained + 2 && Fake::released == released + 1 && Fake::live.size() == 1);
    Fake::fail_at = 1; // growth fails: empty, capacity 0, the old block released exactly once
    CHECK(a.reserve(1000) != Fake::ok);
    CHECK(empty(a) && Fake::live.empty() && Fake::released == released + 2 && Fake::double_release == 0);
    CHECK(a.reserve(65) == Fake::ok && a.count() == 65); // no stale capacity: the old size is obtained again
    CHECK(Fake::obtained == obtained + 3);
}

// A feature's first use as the library writes it: the buffers in one struct, allocated one after the other; on a failure the
// struct is reset.
struct Feature {
    Buf<unsigned char> desc, data;
    Buf<float> table;
    Buf<long long> rec;
    size_t bytes() const { return desc.bytes() + data.bytes() + table.bytes() + rec.bytes(); }
    int first_use()
    {
        int e = desc.alloc(48);
        if (e == Fake::ok)
            e = table.alloc(12, true);
        if (e == Fake::ok)
            e = rec.alloc(6, true);
        if (e == Fake::ok)
            e = data.reserve(100);
        if (e != Fake::ok)
            *this = Feature();
        return e;
    }
};

void all_or_nothing()
{
    for (int k = 1; k <= 4; ++k) {
        Feature f;
        Fake::fail_at = k;
        CHECK(f.first_use() != Fake::ok);
        CHECK(Fake::live.empty() && empty(f.desc) && empty(f.data) && empty(f.table) && empty(f.rec) && f.bytes() == 0);
        CHECK(f.first_use() == Fake::ok && Fake::live.size() == 4); // the retry starts from nothing
    }
    CHECK(Fake::live.empty() && Fake::double_release == 0);
}

void bytes_follow_the_buffers()
{
    Feature f;
    CHECK(f.bytes() == 0);
    CHECK(f.first_use() == Fake::ok);
    CHECK(f.bytes() == 48 + 100 + 12 * sizeof(float) + 6 * sizeof(long long));
    CHECK(f.data.reserve(50) == Fake::ok && f.bytes() == 48 + 100 + 48 + 48); // no growth: the same sum
    CHECK(f.data.reserve(4096) == Fake::ok && f.bytes() == 48 + 4096 + 48 + 48);
    Fake::fail_at = 1;
    CHECK(f.data.reserve(8192) != Fake::ok && f.bytes() == 48 + 0 + 48 + 48); // a buffer that is gone is not counted
    f = Feature();
    CHECK(f.bytes() == 0 && Fake::live.empty());
}

} // namespace

int main()
{
    life_of_a_buffer();
    reserve_grows_only();
    all_or_nothing();
    bytes_follow_the_buffers();
    CHECK(Fake::live.empty() && Fake::obtained == Fake::released && Fake::double_release == 0 && Fake::fail_at == 0);
    if (failures)
        return fprintf(stderr, "mem_check: %d violation(s)\n", failures), 1;
    printf("mem_check ok: %d blocks obtained and released\n", Fake::obtained);
    return 0;
}
