// vtk_output.hpp — ParaView/VisIt output of the `-paraview` dumps: VTK XML files of linear cells over the lattice values
// lgh_sample_fields produces (stands in for the reference's VisItDataCollection, /root/reference/laghos.cpp:691-701,
// :845-871; the layout follows what MFEM's ParaViewDataCollection does with its levels of detail).  Host only, no GPU
// code, no MFEM: a high-order zone becomes R^dim linear cells on its (R+1)^dim lattice points, points duplicated zone
// by zone so that the discontinuous fields are exact.  DESIGN.md §7b.
#pragma once
#include <cstdint>
#include <ostream>
#include <sstream>
#include <string>
#include <vector>

namespace laghos
{

// mkdir -p
void MakeDirs(const std::string &dir);

// the arrays of the appended block, in file order: a DataArray element in the header, UInt64 byte count + data behind it
struct Appended
{
   struct Block { const void *data; uint64_t bytes; };
   std::vector<Block> blocks;
   uint64_t offset = 0;
   std::string Array(const char *type, const char *name, int ncomp, const void *data, uint64_t bytes, const char *extra = "")
   {
      std::ostringstream os;
      os << "<DataArray type=\"" << type << "\" Name=\"" << name << "\"";
      if (ncomp > 0) { os << " NumberOfComponents=\"" << ncomp << "\""; }
      os << extra << " format=\"appended\" offset=\"" << offset << "\"/>\n";
      blocks.push_back({data, bytes});
      offset += sizeof(uint64_t) + bytes;
      return os.str();
   }
   void Write(std::ostream &f) const
   {
      f << "<AppendedData encoding=\"raw\">\n_";
      for (const Block &b : blocks)
      {
         f.write(reinterpret_cast<const char *>(&b.bytes), sizeof(uint64_t));
         f.write(reinterpret_cast<const char *>(b.data), (std::streamsize)b.bytes);
      }
      f << "\n</AppendedData>\n";
   }
};

// "cycle_<6 digits>.vtu", with ".<rank>" in front of the extension on several ranks
std::string VtuName(int cycle, int nranks, int rank);
std::string PvtuName(int cycle);

// One UnstructuredGrid piece <dir>/VtuName(): NP = NE * R1^dim points, structure of arrays as lgh_sample_fields writes
// them (x[c * NP + pt], v[c * NP + pt], e[pt], rho[pt], p[pt]; pt = e * R1^dim + rx + R1 * (ry + R1 * rz)).
// PointData density, velocity, specific_internal_energy, pressure (Float64); CellData zone (the caller's zone id) and
// rank (Int32); FieldData TIME, CYCLE.  Little endian, UInt64 headers, every array in one raw appended block.
bool WriteVtu(const std::string &dir, int dim, int NE, int R1, const double *x, const double *v, const double *e,
              const double *rho, const double *p, int cycle, double time, int rank, int nranks);
// The same piece with further PointData arrays behind the four standing ones, in the order given: each `components`
// Float64 values per point, point by point (data[components * pt + c]).  No extras: the bytes of WriteVtu.
struct VtuField
{
   std::string name;
   int components;
   const double *data;
};
bool WriteVtuFields(const std::string &dir, int dim, int NE, int R1, const double *x, const double *v, const double *e,
                    const double *rho, const double *p, const std::vector<VtuField> &extra, int cycle, double time, int rank,
                    int nranks);
// <dir>/PvtuName(): the pieces of all ranks of one cycle
bool WritePvtu(const std::string &dir, int cycle, double time, int nranks);
// ... whose pieces carry the extra arrays (name and components are read, data is not)
bool WritePvtuFields(const std::string &dir, int cycle, double time, int nranks, const std::vector<VtuField> &extra);
// One piece of a surface or slice dump (`-pv-surface`, `-pv-slice`) <dir>/VtuName(): the lattices of nfaces zone
// faces, faces[2k] = zone, faces[2k + 1] = local face 2 axis + side, NPt = nfaces * R1^(dim-1) points in the layout of
// lgh_sample_faces (x[c * NPt + pt], ..., an[c * NPt + pt]; pt = k * R1^(dim-1) + r_b + R1 * r_c), duplicated face by face.
// Cells: R^2 VTK_QUAD per face in 3D, R VTK_LINE in 2D, corners ordered so that the cell's normal (right-hand rule; in 2D
// the tangent turned clockwise) points out of the zone where det J > 0.  PointData: the four standing arrays, `extra` as
// WriteVtuFields takes it, then area_normal (3 components); CellData zone, face, rank (Int32); FieldData TIME, CYCLE.  The raw
// appended layout of WriteVtuFields.  nfaces == 0 writes an empty piece (the arrays may then be null).
bool WriteVtuFaces(const std::string &dir, int dim, int nfaces, const int *faces, int R1, const double *x, const double *v,
                   const double *e, const double *rho, const double *p, const std::vector<VtuField> &extra, const double *an, int cycle,
                   double time, int rank, int nranks);
// <dir>/PvtuName() for such pieces
bool WritePvtuFaces(const std::string &dir, int cycle, double time, int nranks, const std::vector<VtuField> &extra);
// One piece of a contour dump (`-pv-iso`, `-pv-plane`) <dir>/VtuName(): nprims primitives of dim vertices each -
// VTK_TRIANGLE in 3D, VTK_LINE in 2D - on NPt = dim * nprims points of their own (vertex j of primitive q is point dim q + j), in
// the layout of LagrangianHydroOperator::Contour (x[c * NPt + pt], v[c * NPt + pt], e[pt], rho[pt], p[pt]).  PointData: the four
// standing arrays, then `extra` as WriteVtuFields takes it; CellData zone[q] and rank (Int32); FieldData TIME, CYCLE and ISO_VALUE
// (the value of the field, or D of a plane).  The raw appended layout of WriteVtuFields.  nprims == 0 writes an empty piece (the
// arrays may then be null).
bool WriteVtuContour(const std::string &dir, int dim, long nprims, const int *zone, const double *x, const double *v, const double *e,
                     const double *rho, const double *p, const std::vector<VtuField> &extra, double iso_value, int cycle, double time, int rank,
                     int nranks);
// <dir>/PvtuName() for such pieces
bool WritePvtuContour(const std::string &dir, int cycle, double time, int nranks, const std::vector<VtuField> &extra);
// The collection <pvd_path>: one DataSet per dump so far, file = <rel_dir>/<piece or .pvtu>
bool WritePvd(const std::string &pvd_path, const std::string &rel_dir, const std::vector<double> &times,
              const std::vector<int> &cycles, int nranks);

} // namespace laghos
