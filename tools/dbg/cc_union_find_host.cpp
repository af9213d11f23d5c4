// Host model of the labelling of psnerf_amd/csrc/meshclean.hip: cc_find / cc_link with the kernel's control flow on std::atomic (relaxed),
// threads in place of workgroups, against a sequential union-find.  A stand-alone program for ThreadSanitizer (no GPU, no Python):
//     g++ -O1 -g -fsanitize=thread -std=c++17 -pthread tools/dbg/cc_union_find_host.cpp -o /tmp/cc_uf && /tmp/cc_uf
// Inputs: a ribbon of 4096 triangles (i, i + 1, i + 2) with shuffled vertex ids (deep forests, long walks) and a random sparse mesh of
// 20000 vertices / 30000 faces with duplicated and degenerate faces (many components, contended roots).  Exit status 0 = every run of
// every input gave the sequential labels.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

static std::atomic<int>* parent;
static std::atomic<int> status{0};

static int cc_find(int x, int64_t bound) {
    int cur = x;
    for (int64_t step = 0; step <= bound; ++step) {
        const int p = parent[cur].load(std::memory_order_relaxed);
        if (p == cur) return cur;
        const int gp = parent[p].load(std::memory_order_relaxed);
        if (gp != p) parent[cur].store(gp, std::memory_order_relaxed);
        cur = gp;
    }
    return -1;
}

static bool cc_link(int u, int v, int64_t bound) {
    int a = cc_find(u, bound), b = cc_find(v, bound);
    for (int64_t tries = 0; tries <= bound; ++tries) {
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (parent[hi].compare_exchange_strong(seen, lo, std::memory_order_relaxed)) return true;
        a = cc_find(seen, bound);
        b = lo;
    }
    return false;
}

static std::vector<int> sequential(const std::vector<int>& faces, int n_vertices) {
    std::vector<int> p(n_vertices);
    std::iota(p.begin(), p.end(), 0);
    auto find = [&](int x) {
        while (p[x] != x) x = p[x] = p[p[x]];
        return x;
    };
    for (size_t f = 0; f < faces.size() / 3; ++f)
        for (int e = 0; e < 2; ++e) {
            const int a = find(faces[3 * f + e]), b = find(faces[3 * f + e + 1]);
            if (a != b) p[std::max(a, b)] = std::min(a, b);
        }
    for (int v = 0; v < n_vertices; ++v) p[v] = find(v);
    return p;
}

static int run(const char* name, const std::vector<int>& faces, int n_vertices, int n_threads, int repeats) {
    const std::vector<int> want = sequential(faces, n_vertices);
    const int64_t n_faces = (int64_t)faces.size() / 3;
    int bad = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        parent = new std::atomic<int>[n_vertices];
        for (int v = 0; v < n_vertices; ++v) parent[v].store(v);
        status.store(0);
        std::vector<std::thread> threads;
        for (int t = 0; t < n_threads; ++t)
            threads.emplace_back([&, t] {
                for (int64_t block = t; block * 64 < n_faces; block += n_threads)   // a "wave" of 64 faces at a time, interleaved
                    for (int64_t f = block * 64; f < n_faces && f < block * 64 + 64; ++f) {
                        const int i = faces[3 * f], j = faces[3 * f + 1], k = faces[3 * f + 2];
                        bool ok = true;
                        if (i != j) ok = cc_link(i, j, n_vertices);
                        if (ok && j != k) ok = cc_link(j, k, n_vertices);
                        if (!ok) status.fetch_or(2);
                    }
            });
        for (auto& t : threads) t.join();
        int64_t wrong = 0, deepest = 0;
        for (int v = 0; v < n_vertices; ++v) {   // the flatten launch
            int cur = v;
            int64_t depth = 0;
            while (parent[cur].load() != cur) { cur = parent[cur].load(); ++depth; }
            wrong += cur != want[v];
            deepest = std::max(deepest, depth);
        }
        if (wrong || status.load()) { ++bad; printf("%s run %d: %lld wrong labels, status %d\n", name, rep, (long long)wrong, status.load()); }
        if (rep == 0) printf("%s: %d vertices, %lld faces, deepest walk before the flatten %lld\n", name, n_vertices, (long long)n_faces, (long long)deepest);
        delete[] parent;
    }
    printf("%s: %d of %d runs differ from the sequential labels\n", name, bad, repeats);
    return bad;
}

int main() {
    std::mt19937 g(0);
    std::vector<int> ids(4098);
    std::iota(ids.begin(), ids.end(), 0);
    std::shuffle(ids.begin(), ids.end(), g);
    std::vector<int> ribbon;
    for (int i = 0; i < 4096; ++i)
        for (int c = 0; c < 3; ++c) ribbon.push_back(ids[i + c]);
    const int n_v = 20000;
    std::vector<int> sparse;
    std::uniform_int_distribution<int> any(0, n_v - 1), near(-3, 3);
    for (int f = 0; f < 30000; ++f) {
        const int a = any(g);
        const int b = std::min(std::max(a + near(g), 0), n_v - 1), c = (f % 7 == 0) ? any(g) : std::min(std::max(a + near(g), 0), n_v - 1);
        sparse.insert(sparse.end(), {a, b, c});
        if (f % 50 == 0) sparse.insert(sparse.end(), {a, b, c});   // a duplicated face
    }
    const int bad = run("ribbon", ribbon, 4098 + 4, 16, 20) + run("sparse", sparse, n_v, 16, 20);
    return bad != 0;
}
