// tests/cpp/elev_move_main.cpp -- stand-alone driver of the elevation restatement's Move (oracle/elev_oracle.cpp), meant to be
// compiled together with it under -fsanitize=address,undefined (tests/test_oracle_elev.py does).  It jumps a filled map by
// +-L, +-(2L+3) and -50L cells on each axis, for both parities of L: shifts the reference's `indexShift >= length` test sends
// into a partial clear longer than the map.  Every such jump must leave an empty map, the frame of a plain wrap-around, and
// no sanitizer report.
#include <cstdio>
#include <vector>

extern "C" {
void* orc_elev_create(int length, float resolution, float mahal_thr, float obstacle_thr);
void orc_elev_destroy(void* h);
int orc_elev_move(void* h, const float* pos3, float* central, int* start, float* aligned_shift);
void orc_elev_fuse(void* h, int n, const int* index, const int* cR, const int* cG, const int* cB, const float* inten, const float* ph,
                   const float* pv);
void orc_elev_get(void* h, int which, float* out);
}

static int fails = 0;

static void jump(int L, int axis, int cells)
{
    const float res = 0.5f;
    void* m = orc_elev_create(L, res, 2.0f, 0.6f);
    const int n = L * L;
    std::vector<int> idx(n), col(n, 7);
    std::vector<float> inten(n, 0.5f), h(n), v(n, 0.01f);
    for (int i = 0; i < n; ++i) { idx[i] = i; h[i] = 0.01f * (float)(i + 1); }
    orc_elev_fuse(m, n, idx.data(), col.data(), col.data(), col.data(), inten.data(), h.data(), v.data());
    float pos[3] = {0, 0, 1.0f}, central[2], aligned[2];
    int start[2];
    pos[axis] = res * (float)cells;
    const int st = orc_elev_move(m, pos, central, start, aligned);
    std::vector<float> e(n), tr(n);
    orc_elev_get(m, 1, e.data());
    orc_elev_get(m, 4, tr.data());
    int left = 0;
    for (int i = 0; i < n; ++i) left += e[i] != -10.0f || tr[i] != -10.0f;
    const int want_start = ((-cells) % L + L) % L;
    const bool ok = st == 0 && left == 0 && start[axis] == want_start && start[1 - axis] == 0 && aligned[axis] == res * (float)cells;
    std::printf("L=%d axis=%d shift=%d: status %d, %d cells left, start %d (want %d)%s\n", L, axis, cells, st, left, start[axis],
                want_start, ok ? "" : "  FAILED");
    fails += !ok;
    orc_elev_destroy(m);
}

int main()
{
    for (int L : {8, 9})
        for (int axis : {0, 1})
            for (int cells : {L, -L, L + 1, -(L + 1), 2 * L + 3, -(2 * L + 3), -50 * L}) jump(L, axis, cells);
    std::printf(fails ? "elev move: %d FAILED\n" : "elev move: all jumps clear the map\n", fails);
    return fails ? 1 : 0;
}
