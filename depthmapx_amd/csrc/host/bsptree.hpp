// bsptree.hpp -- the binary space partition of the drawing lines that the isovist analysis walks.
// Restates VGAIsovist::makeBSPtree (salalib/vgamodules/vgaisovist.cpp:92-129) and BSPTree::make,
// pickMidpointLine and makeLines (genlib/bsptree.cpp:34-182), flattened to arrays.
//
// Sets of more than 3 lines split at the reference's pick: the line whose midpoint is nearest the set's mean
// midpoint, tall lines under a wide (or no) parent and wide lines under a tall one.  For sets of at most 3
// lines the reference draws from its global LCG (pafrand() % size), so its tree depends on the history of the
// process; here the FIRST line of the set is taken.  The isovists do not depend on that choice (any BSP gives
// the same front-to-back order of what a cell can see) -- only on ties the reference itself does not fix.
//
// Built iteratively, as in the reference: a 500-piece arc gives a 500-deep tree.  `depth` and the parent
// links are recorded so that a walk needs no stack sized by guesswork.
#pragma once
#include <cstdint>
#include <vector>

#include "geometry.hpp"

namespace dmx {

struct BspTree {
    std::vector<double> seg;       // [n][4] start.x, start.y, end.x, end.y (Line::start() / end())
    std::vector<int32_t> tag;      // [n] index of the input line the piece comes from
    std::vector<int32_t> left, right, parent;   // [n] node index or -1
    int depth = 0;                 // nodes on the longest root-to-leaf path
    int64_t nodes() const { return (int64_t)tag.size(); }
};

// lines: [n][4] x1, y1, x2, y2; zero-length lines are dropped (vgaisovist.cpp:106-110).
void bsp_build(const double* lines, int64_t nlines, BspTree& out);

}  // namespace dmx
