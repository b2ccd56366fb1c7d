// pack_fit_dump.cpp -- the packing rule of the leftovers (csrc/pack_fit.hpp) run on arrays read from standard input:
// the stand-alone program of tests/test_pack_fit_cpu.py.  One array of leftovers per line; for each the program prints
//   N <cells> <packs of the count pass> <packs of the write pass>
//   P <cell> <cell> <cell> <cell>        one line per pack, in pack order (-1: unused place)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pack_fit.hpp"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<int> r;
        for (int v; in >> v;) r.push_back(v);
        const int n = (int)r.size();
        const int counted = psamd::pack_fit(r.data(), n, nullptr);
        std::vector<int> out((size_t)psamd::PACK_GROUPS * (size_t)counted, -2);      // exactly the count pass's room
        const int written = psamd::pack_fit(r.data(), n, out.data());
        std::printf("N %d %d %d\n", n, counted, written);
        for (int p = 0; p < counted; p++)
            std::printf("P %d %d %d %d\n", out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
    }
    return 0;
}
