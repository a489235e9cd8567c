// dmx_salalib.h -- reference-side binding: route salalib's makeGraph and VGA global to libdmx.so.
//
// A maintainer adds integration/dmx_salalib.cpp to salalib and calls these at the top of the
// methods they accelerate (INTEGRATION.md shows the two-line hooks):
//   PointMap::sparkGraph2        salalib/pointdata.cpp:1246-1341
//   VGAVisualGlobal::run         salalib/vgamodules/vgavisualglobal.cpp:23-216
//   VGAThroughVision::run        salalib/vgamodules/vgathroughvision.cpp:27-104
//   VGAIsovist::run              salalib/vgamodules/vgaisovist.cpp:24-90
// Each returns true when the engine ran the analysis and `map` now holds exactly what the reference
// method would have left in it (the point states, nodes, attribute columns and statistics, through
// the reference's own PointMap::read of the engine's byte-identical PointMap::write image), and false
// when the map is outside what the engine reproduces exactly (no GPU, a grid set with a non-zero
// offset, merge links); the caller then runs its own code.  Cancellation through the Communicator
// throws Communicator::CancelledException as the reference does; engine errors throw
// depthmapX::RuntimeException.
#pragma once

#include <utility>
#include <vector>

class Communicator;
class MetaGraph;
class Point2f;
class PointMap;

namespace dmxsala {

bool sparkGraph2(PointMap& map, Communicator* comm, bool boundarygraph, double maxdist);
bool vgaVisualGlobal(PointMap& map, Communicator* comm, double radius, bool gates_only, bool simple_version);
// VGAThroughVision::run (salalib/vgamodules/vgathroughvision.cpp:27-104); false also for a map with the gate
// column __Internal_Gate (the gate-counting branch, :61-74) or one that already has "Through vision".
bool vgaThroughVision(PointMap& map, Communicator* comm);
// VGAIsovist::run (salalib/vgamodules/vgaisovist.cpp:24-90): the eight isovist columns, the nodes' occlusion bins
// and occ distances, m_hasIsovistAnalysis; false also for a map without drawing lines or one that already has
// "Isovist Area".  Values agree with the reference within 1e-6 relative (the platform's acos / sin / cos).
bool vgaIsovist(PointMap& map, Communicator* comm, bool simple_version);

// MetaGraph::makeIsovist (salalib/mgraph.cpp:491-521) for a batch of points, what depthmapXcli -m ISOVIST loops over
// (runmethods.cpp:635-647): the polygons and attribute values come from one dmx_isovists call, the "Isovists" data
// map from the reference's own ShapeMap::makePolyShape / setCentroid and AttributeRow::setValue.  angles: (startangle,
// endangle) per point as makeIsovist takes them, or empty for full circles.  Returns what makeIsovist returns: 0
// nothing made (no GPU, no drawing lines: the caller runs its own loop), 1 isovists made, 2 and the data map added.
// Polygon vertices on a wall the BSP tree cuts depend on the tree, as they do in the reference (include/dmx.h).
int makeIsovists(MetaGraph& mg, const std::vector<Point2f>& points, const std::vector<std::pair<double, double>>& angles,
                 bool simple_version);

// Test hooks (integration/bind_check.cpp): the PointMap <-> PointMap::write image conversions the two
// calls are built on.
bool saveMap(PointMap& map, void* bytes_out /* std::string* */);
bool loadMap(PointMap& map, const void* bytes /* const std::string* */);

}  // namespace dmxsala
