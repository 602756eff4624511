// The owner types of hierdiff_amd/csrc/mem.hpp on their own: no HIP runtime, the two raw functions over malloc / free with
// counters of this program and a switch that makes the n-th allocation fail.  Built with -fsanitize=address,undefined and run by
// tests/test_mem_owner_cpu.py; a failed check prints its line and the program exits 1.
#include "../hierdiff_amd/csrc/mem.hpp"

#include <cstdio>
#include <cstdlib>

static long long g_count = 0, g_bytes = 0, g_allocs_made = 0, g_frees = 0;
static long long g_fail_at = -1;               // the allocation with this ordinal (counted from 0, from the last arm()) fails
static void arm(long long nth) { g_fail_at = nth; g_allocs_made = 0; }

int hd_raw_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (g_allocs_made++ == g_fail_at) return HD_E_NOMEM;
    *p = std::malloc(bytes);
    if (!*p) return HD_E_NOMEM;
    ++g_count; g_bytes += (long long)bytes;
    return HD_OK;
}

void hd_raw_free(void* p, size_t bytes) {
    std::free(p);
    --g_count; g_bytes -= (long long)bytes; ++g_frees;
}

static int g_failed = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed = 1; } \
    } while (0)

static int g_destroyed = 0;
static int fake_destroy(int* h) { ++g_destroyed; delete h; return 0; }
using Handle = Owned<int*, fake_destroy>;

struct Three {                                 // the shape of RestraintState / SteerAttach: owners next to plain members
    int n = 0;
    DevBuf<float> a;
    DevBuf<int> b;
    DevBuf<double> c;
    int fill(size_t k) {
        int r = a.alloc(k);
        if (r == HD_OK) r = b.alloc(k);
        if (r == HD_OK) r = c.alloc(k);
        if (r == HD_OK) n = (int)k;
        return r;
    }
};

int main() {
    {   // an empty owner frees nothing
        DevBuf<float> e;
        CHECK(!e && e.capacity() == 0 && e.bytes() == 0);
        e.release();
    }
    CHECK(g_count == 0 && g_frees == 0);

    {   // allocate then destroy is balanced; count 0 allocates one element
        DevBuf<float> a;
        CHECK(a.alloc(10) == HD_OK && a && a.capacity() == 10 && g_count == 1 && g_bytes == 40);
        static_cast<float*>(a)[9] = 1.f;
        DevBuf<long long> z;
        CHECK(z.alloc(0) == HD_OK && z && z.capacity() == 1 && g_bytes == 48);
        static_cast<long long*>(z)[0] = 7;
    }
    CHECK(g_count == 0 && g_bytes == 0 && g_frees == 2);

    {   // move construction empties the source; move assignment frees the target's old block; self-move is safe
        DevBuf<int> a;
        CHECK(a.alloc(4) == HD_OK);
        int* pa = a;
        DevBuf<int> b(std::move(a));
        CHECK(!a && a.capacity() == 0 && static_cast<int*>(b) == pa && b.capacity() == 4 && g_count == 1);
        DevBuf<int> c;
        CHECK(c.alloc(8) == HD_OK && g_count == 2);
        const long long frees = g_frees;
        c = std::move(b);
        CHECK(!b && static_cast<int*>(c) == pa && c.capacity() == 4 && g_count == 1 && g_frees == frees + 1 && g_bytes == 16);
        DevBuf<int>& self = c;
        c = std::move(self);
        CHECK(static_cast<int*>(c) == pa && c.capacity() == 4 && g_count == 1);
        static_cast<int*>(c)[3] = 3;
    }
    CHECK(g_count == 0 && g_bytes == 0);

    {   // allocate-once does not reallocate; grow keeps the address while the capacity suffices, otherwise moves and frees
        DevBuf<float> a;
        CHECK(a.alloc_once(6) == HD_OK);
        float* p = a;
        CHECK(a.alloc_once(600) == HD_OK && static_cast<float*>(a) == p && a.capacity() == 6 && g_count == 1);
        bool moved = false;
        CHECK(a.grow(6, &moved) == HD_OK && !moved && static_cast<float*>(a) == p);
        CHECK(a.grow(2, &moved) == HD_OK && !moved && static_cast<float*>(a) == p && a.capacity() == 6);
        const long long frees = g_frees;
        CHECK(a.grow(7, &moved) == HD_OK && moved && a.capacity() == 7 && g_count == 1 && g_frees == frees + 1 && g_bytes == 28);
        static_cast<float*>(a)[6] = 2.f;
        DevBuf<float> e;                       // an empty one grows into its first block
        moved = false;
        CHECK(e.grow(0, &moved) == HD_OK && moved && e.capacity() == 1 && g_count == 2);
        a.release();
        CHECK(!a && g_count == 1);
    }
    CHECK(g_count == 0 && g_bytes == 0);

    {   // a failing allocation returns HD_E_NOMEM and leaves the owner empty - a fresh one, and one that held a block
        DevBuf<float> a;
        arm(0);
        CHECK(a.alloc(5) == HD_E_NOMEM && !a && a.capacity() == 0 && g_count == 0);
        arm(-1);
        CHECK(a.alloc(5) == HD_OK && g_count == 1);
        arm(0);
        bool moved = false;
        CHECK(a.grow(50, &moved) == HD_E_NOMEM && !a && a.capacity() == 0 && g_count == 0);
        arm(-1);
    }
    CHECK(g_count == 0 && g_bytes == 0);

    {   // a struct of three owners whose second allocation fails is cleaned up by its destructor
        Three t;
        arm(1);
        CHECK(t.fill(16) == HD_E_NOMEM && t.a && !t.b && !t.c && t.n == 0 && g_count == 1);
        arm(-1);
    }
    CHECK(g_count == 0 && g_bytes == 0);

    {   // move-assigning a default-constructed struct over a filled one frees everything
        Three t;
        CHECK(t.fill(16) == HD_OK && g_count == 3 && g_bytes == 16 * (4 + 4 + 8));
        t = Three{};
        CHECK(g_count == 0 && g_bytes == 0 && !t.a && !t.b && !t.c && t.n == 0);
        // ... and all-or-none: locals moved in once every allocation succeeded
        Three local;
        arm(2);
        CHECK(local.fill(4) == HD_E_NOMEM);
        arm(-1);
        CHECK(!t.a && g_count == 2);
        CHECK(local.fill(4) == HD_OK);
        t = std::move(local);
        CHECK(t.a && t.b && t.c && t.n == 4 && !local.a && g_count == 3);
    }
    CHECK(g_count == 0 && g_bytes == 0);

    {   // the handle owner: destroys once, adopt() drops what it held, a moved-from one destroys nothing
        Handle e;
        CHECK(!e);
        e.adopt(new int(1));
        CHECK(e && g_destroyed == 0);
        Handle f(std::move(e));
        CHECK(!e && f);
        f.adopt(new int(2));
        CHECK(g_destroyed == 1);
        Handle g;
        g = std::move(f);
        Handle& self = g;
        g = std::move(self);
        CHECK(g && !f && g_destroyed == 1);
        g.reset();
        CHECK(!g && g_destroyed == 2);
        g.reset();
    }
    CHECK(g_destroyed == 2);

    CHECK(g_count == 0 && g_bytes == 0);       // the counters read 0 at exit
    if (!g_failed) std::printf("mem owners: ok\n");
    return g_failed;
}
