// vtk_output.cpp — VTK XML writers of the `-paraview` dumps (vtk_output.hpp).
#include "vtk_output.hpp"

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <sstream>
#include <sys/stat.h>

namespace laghos
{

void MakeDirs(const std::string &dir)
{
   for (size_t p = 1; p <= dir.size(); p++)
   {
      if (p == dir.size() || dir[p] == '/') { (void)::mkdir(dir.substr(0, p).c_str(), 0777); }
   }
}

static std::string CycleTag(int cycle)
{
   char buf[32];
   std::snprintf(buf, sizeof(buf), "cycle_%06d", cycle);
   return buf;
}
std::string VtuName(int cycle, int nranks, int rank)
{
   std::string s = CycleTag(cycle);
   if (nranks > 1) { s += "." + std::to_string(rank); }
   return s + ".vtu";
}
std::string PvtuName(int cycle) { return CycleTag(cycle) + ".pvtu"; }

namespace
{

// c-th component of point pt of a dim-component structure of arrays, zero above dim
std::vector<double> Interleave3(const double *soa, int dim, size_t NP)
{
   std::vector<double> a(3 * NP, 0.0);
   for (int c = 0; c < dim; c++)
   {
      for (size_t i = 0; i < NP; i++) { a[3 * i + c] = soa[c * NP + i]; }
   }
   return a;
}

const char *kPointArrays[4][2] = {{"density", "1"}, {"velocity", "3"}, {"specific_internal_energy", "1"}, {"pressure", "1"}};

} // namespace

bool WriteVtu(const std::string &dir, int dim, int NE, int R1, const double *x, const double *v, const double *e,
              const double *rho, const double *p, int cycle, double time, int rank, int nranks)
{
   return WriteVtuFields(dir, dim, NE, R1, x, v, e, rho, p, {}, cycle, time, rank, nranks);
}

bool WriteVtuFields(const std::string &dir, int dim, int NE, int R1, const double *x, const double *v, const double *e,
                    const double *rho, const double *p, const std::vector<VtuField> &extra, int cycle, double time, int rank,
                    int nranks)
{
   if (dim < 1 || dim > 3 || NE < 0 || R1 < 2 || !x || !v || !e || !rho || !p) { return false; }
   for (const VtuField &f : extra)
   {
      if (f.name.empty() || f.components < 1 || !f.data) { return false; }
   }
   const int R = R1 - 1;
   size_t NPZ = 1, NCZ = 1;
   for (int a = 0; a < dim; a++) { NPZ *= R1; NCZ *= R; }
   const size_t NP = (size_t)NE * NPZ, NC = (size_t)NE * NCZ;
   const int nv = 1 << dim; // corners of a cell
   const std::vector<double> pts = Interleave3(x, dim, NP), vel = Interleave3(v, dim, NP);
   // R^dim linear cells per zone on the zone's own lattice points, corners in VTK's order (VTK_LINE 3, VTK_QUAD 9,
   // VTK_HEXAHEDRON 12: counter-clockwise in the bottom plane, then the top plane)
   static const int corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
   std::vector<int64_t> conn(NC * nv), offs(NC);
   std::vector<uint8_t> types(NC, (uint8_t)(dim == 3 ? 12 : (dim == 2 ? 9 : 3)));
   std::vector<int32_t> zone(NC), rnk(NC, (int32_t)rank);
   const int Ry = dim > 1 ? R : 1, Rz = dim > 2 ? R : 1;
   size_t cell = 0;
   for (int z = 0; z < NE; z++)
   {
      for (int cz = 0; cz < Rz; cz++)
         for (int cy = 0; cy < Ry; cy++)
            for (int cx = 0; cx < R; cx++, cell++)
            {
               for (int k = 0; k < nv; k++)
               {
                  const int rx = cx + corner[k][0], ry = cy + corner[k][1], rz = cz + corner[k][2];
                  conn[cell * nv + k] = (int64_t)((size_t)z * NPZ + rx + (size_t)R1 * (ry + (size_t)R1 * rz));
               }
               offs[cell] = (int64_t)((cell + 1) * nv);
               zone[cell] = z;
            }
   }
   const int32_t cyc = cycle;
   Appended ap;
   std::ostringstream h;
   h << "<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
        "header_type=\"UInt64\">\n<UnstructuredGrid>\n<FieldData>\n";
   h << ap.Array("Float64", "TIME", 0, &time, sizeof(double), " NumberOfTuples=\"1\"");
   h << ap.Array("Int32", "CYCLE", 0, &cyc, sizeof(int32_t), " NumberOfTuples=\"1\"");
   h << "</FieldData>\n<Piece NumberOfPoints=\"" << NP << "\" NumberOfCells=\"" << NC << "\">\n<Points>\n";
   h << ap.Array("Float64", "Points", 3, pts.data(), pts.size() * sizeof(double));
   h << "</Points>\n<Cells>\n";
   h << ap.Array("Int64", "connectivity", 0, conn.data(), conn.size() * sizeof(int64_t));
   h << ap.Array("Int64", "offsets", 0, offs.data(), offs.size() * sizeof(int64_t));
   h << ap.Array("UInt8", "types", 0, types.data(), types.size());
   h << "</Cells>\n<PointData Scalars=\"density\" Vectors=\"velocity\">\n";
   h << ap.Array("Float64", "density", 1, rho, NP * sizeof(double));
   h << ap.Array("Float64", "velocity", 3, vel.data(), vel.size() * sizeof(double));
   h << ap.Array("Float64", "specific_internal_energy", 1, e, NP * sizeof(double));
   h << ap.Array("Float64", "pressure", 1, p, NP * sizeof(double));
   for (const VtuField &f : extra) { h << ap.Array("Float64", f.name.c_str(), f.components, f.data, NP * f.components * sizeof(double)); }
   h << "</PointData>\n<CellData>\n";
   h << ap.Array("Int32", "zone", 1, zone.data(), zone.size() * sizeof(int32_t));
   h << ap.Array("Int32", "rank", 1, rnk.data(), rnk.size() * sizeof(int32_t));
   h << "</CellData>\n</Piece>\n</UnstructuredGrid>\n";
   MakeDirs(dir);
   std::ofstream f((dir + "/" + VtuName(cycle, nranks, rank)).c_str(), std::ios::binary);
   if (!f) { return false; }
   f << h.str();
   ap.Write(f);
   f << "</VTKFile>\n";
   f.close();
   return !f.fail();
}

bool WritePvtu(const std::string &dir, int cycle, double time, int nranks) { return WritePvtuFields(dir, cycle, time, nranks, {}); }

bool WritePvtuFields(const std::string &dir, int cycle, double time, int nranks, const std::vector<VtuField> &extra)
{
   for (const VtuField &f : extra)
   {
      if (f.name.empty() || f.components < 1) { return false; }
   }
   MakeDirs(dir);
   std::ofstream f((dir + "/" + PvtuName(cycle)).c_str());
   if (!f) { return false; }
   f << std::setprecision(17);
   f << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PUnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
        "header_type=\"UInt64\">\n<PUnstructuredGrid GhostLevel=\"0\">\n";
   f << "<!-- cycle " << cycle << ", time " << time << " -->\n";
   f << "<PPoints>\n<PDataArray type=\"Float64\" Name=\"Points\" NumberOfComponents=\"3\"/>\n</PPoints>\n";
   f << "<PPointData Scalars=\"density\" Vectors=\"velocity\">\n";
   for (auto &a : kPointArrays)
   {
      f << "<PDataArray type=\"Float64\" Name=\"" << a[0] << "\" NumberOfComponents=\"" << a[1] << "\"/>\n";
   }
   for (const VtuField &a : extra)
   {
      f << "<PDataArray type=\"Float64\" Name=\"" << a.name << "\" NumberOfComponents=\"" << a.components << "\"/>\n";
   }
   f << "</PPointData>\n<PCellData>\n<PDataArray type=\"Int32\" Name=\"zone\" NumberOfComponents=\"1\"/>\n"
        "<PDataArray type=\"Int32\" Name=\"rank\" NumberOfComponents=\"1\"/>\n</PCellData>\n";
   for (int r = 0; r < nranks; r++) { f << "<Piece Source=\"" << VtuName(cycle, nranks, r) << "\"/>\n"; }
   f << "</PUnstructuredGrid>\n</VTKFile>\n";
   f.close();
   return !f.fail();
}

bool WriteVtuFaces(const std::string &dir, int dim, int nfaces, const int *faces, int R1, const double *x, const double *v,
                   const double *e, const double *rho, const double *p, const std::vector<VtuField> &extra, const double *an, int cycle,
                   double time, int rank, int nranks)
{
   if (dim < 2 || dim > 3 || nfaces < 0 || R1 < 2) { return false; }
   if (nfaces > 0 && (!faces || !x || !v || !e || !rho || !p || !an)) { return false; }
   for (const VtuField &f : extra)
   {
      if (f.name.empty() || f.components < 1 || (nfaces > 0 && !f.data)) { return false; }
   }
   for (int k = 0; k < nfaces; k++)
   {
      if (faces[2 * k] < 0 || faces[2 * k + 1] < 0 || faces[2 * k + 1] >= 2 * dim) { return false; }
   }
   const int R = R1 - 1;
   const size_t NPF = (dim == 3) ? (size_t)R1 * R1 : (size_t)R1, NCF = (dim == 3) ? (size_t)R * R : (size_t)R;
   const size_t NP = (size_t)nfaces * NPF, NC = (size_t)nfaces * NCF;
   const int nv = (dim == 3) ? 4 : 2; // corners of a cell
   static const double none = 0.0;    // (an empty piece: every block has zero bytes, the pointer is never read)
   const std::vector<double> pts = nfaces ? Interleave3(x, dim, NP) : std::vector<double>(), vel = nfaces ? Interleave3(v, dim, NP) : std::vector<double>(),
                             nrm = nfaces ? Interleave3(an, dim, NP) : std::vector<double>();
   // counter-clockwise in the lattice's (r_b, r_c): the normal e_b x e_c, which is +e_a for a = 0, 2 and -e_a for a = 1; the
   // outward normal is +e_a on side 1, -e_a on side 0 - the other sense runs the corners backwards
   static const int ccw[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
   std::vector<int64_t> conn(NC * nv), offs(NC);
   std::vector<uint8_t> types(NC, (uint8_t)(dim == 3 ? 9 : 3));
   std::vector<int32_t> zone(NC), face(NC), rnk(NC, (int32_t)rank);
   size_t cell = 0;
   for (int k = 0; k < nfaces; k++)
   {
      const int a = faces[2 * k + 1] >> 1, s = faces[2 * k + 1] & 1;
      // 3D: e_b x e_c = +e_a unless a == 1.  2D: the tangent e_b turned clockwise is +e_a for a == 0 (b = y) and -e_a for a == 1
      const bool along = (dim == 3) ? (a != 1) : (a == 0);
      const bool flip = along != (s == 1);
      for (int cc = 0; cc < (dim == 3 ? R : 1); cc++)
         for (int cb = 0; cb < R; cb++, cell++)
         {
            for (int i = 0; i < nv; i++)
            {
               const int j = flip ? (nv - i) % nv : i; // (quads: 0 3 2 1; lines: 0 1 -> 1 0 below)
               const int c2 = (dim == 3) ? ccw[j][0] : (flip ? 1 - i : i), c3 = (dim == 3) ? ccw[j][1] : 0;
               conn[cell * nv + i] = (int64_t)((size_t)k * NPF + (cb + c2) + (size_t)R1 * (cc + c3));
            }
            offs[cell] = (int64_t)((cell + 1) * nv);
            zone[cell] = faces[2 * k];
            face[cell] = faces[2 * k + 1];
         }
   }
   const int32_t cyc = cycle;
   auto ptr = [&](const double *q) { return q ? q : &none; };
   Appended ap;
   std::ostringstream h;
   h << "<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
        "header_type=\"UInt64\">\n<UnstructuredGrid>\n<FieldData>\n";
   h << ap.Array("Float64", "TIME", 0, &time, sizeof(double), " NumberOfTuples=\"1\"");
   h << ap.Array("Int32", "CYCLE", 0, &cyc, sizeof(int32_t), " NumberOfTuples=\"1\"");
   h << "</FieldData>\n<Piece NumberOfPoints=\"" << NP << "\" NumberOfCells=\"" << NC << "\">\n<Points>\n";
   h << ap.Array("Float64", "Points", 3, pts.data(), pts.size() * sizeof(double));
   h << "</Points>\n<Cells>\n";
   h << ap.Array("Int64", "connectivity", 0, conn.data(), conn.size() * sizeof(int64_t));
   h << ap.Array("Int64", "offsets", 0, offs.data(), offs.size() * sizeof(int64_t));
   h << ap.Array("UInt8", "types", 0, types.data(), types.size());
   h << "</Cells>\n<PointData Scalars=\"density\" Vectors=\"velocity\">\n";
   h << ap.Array("Float64", "density", 1, ptr(rho), NP * sizeof(double));
   h << ap.Array("Float64", "velocity", 3, vel.data(), vel.size() * sizeof(double));
   h << ap.Array("Float64", "specific_internal_energy", 1, ptr(e), NP * sizeof(double));
   h << ap.Array("Float64", "pressure", 1, ptr(p), NP * sizeof(double));
   for (const VtuField &f : extra) { h << ap.Array("Float64", f.name.c_str(), f.components, ptr(f.data), NP * f.components * sizeof(double)); }
   h << ap.Array("Float64", "area_normal", 3, nrm.data(), nrm.size() * sizeof(double));
   h << "</PointData>\n<CellData>\n";
   h << ap.Array("Int32", "zone", 1, zone.data(), zone.size() * sizeof(int32_t));
   h << ap.Array("Int32", "face", 1, face.data(), face.size() * sizeof(int32_t));
   h << ap.Array("Int32", "rank", 1, rnk.data(), rnk.size() * sizeof(int32_t));
   h << "</CellData>\n</Piece>\n</UnstructuredGrid>\n";
   MakeDirs(dir);
   std::ofstream f((dir + "/" + VtuName(cycle, nranks, rank)).c_str(), std::ios::binary);
   if (!f) { return false; }
   f << h.str();
   ap.Write(f);
   f << "</VTKFile>\n";
   f.close();
   return !f.fail();
}

bool WritePvtuFaces(const std::string &dir, int cycle, double time, int nranks, const std::vector<VtuField> &extra)
{
   for (const VtuField &f : extra)
   {
      if (f.name.empty() || f.components < 1) { return false; }
   }
   MakeDirs(dir);
   std::ofstream f((dir + "/" + PvtuName(cycle)).c_str());
   if (!f) { return false; }
   f << std::setprecision(17);
   f << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PUnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
        "header_type=\"UInt64\">\n<PUnstructuredGrid GhostLevel=\"0\">\n";
   f << "<!-- cycle " << cycle << ", time " << time << " -->\n";
   f << "<PPoints>\n<PDataArray type=\"Float64\" Name=\"Points\" NumberOfComponents=\"3\"/>\n</PPoints>\n";
   f << "<PPointData Scalars=\"density\" Vectors=\"velocity\">\n";
   for (auto &a : kPointArrays)
   {
      f << "<PDataArray type=\"Float64\" Name=\"" << a[0] << "\" NumberOfComponents=\"" << a[1] << "\"/>\n";
   }
   for (const VtuField &a : extra)
   {
      f << "<PDataArray type=\"Float64\" Name=\"" << a.name << "\" NumberOfComponents=\"" << a.components << "\"/>\n";
   }
   f << "<PDataArray type=\"Float64\" Name=\"area_normal\" NumberOfComponents=\"3\"/>\n";
   f << "</PPointData>\n<PCellData>\n<PDataArray type=\"Int32\" Name=\"zone\" NumberOfComponents=\"1\"/>\n"
        "<PDataArray type=\"Int32\" Name=\"face\" NumberOfComponents=\"1\"/>\n"
        "<PDataArray type=\"Int32\" Name=\"rank\" NumberOfComponents=\"1\"/>\n</PCellData>\n";
   for (int r = 0; r < nranks; r++) { f << "<Piece Source=\"" << VtuName(cycle, nranks, r) << "\"/>\n"; }
   f << "</PUnstructuredGrid>\n</VTKFile>\n";
   f.close();
   return !f.fail();
}

bool WriteVtuContour(const std::string &dir, int dim, long nprims, const int *zone, const double *x, const double *v, const double *e,
                     const double *rho, const double *p, const std::vector<VtuField> &extra, double iso_value, int cycle, double time, int rank,
                     int nranks)
{
   if (dim < 2 || dim > 3 || nprims < 0) { return false; }
   if (nprims > 0 && (!zone || !x || !v || !e || !rho || !p)) { return false; }
   for (const VtuField &f : extra)
   {
      if (f.name.empty() || f.components < 1 || (nprims > 0 && !f.data)) { return false; }
   }
   const size_t NC = (size_t)nprims, NP = NC * dim;
   static const double none = 0.0; // (an empty piece: every block has zero bytes, the pointer is never read)
   const std::vector<double> pts = NC ? Interleave3(x, dim, NP) : std::vector<double>(), vel = NC ? Interleave3(v, dim, NP) : std::vector<double>();
   std::vector<int64_t> conn(NP), offs(NC);
   std::vector<uint8_t> types(NC, (uint8_t)(dim == 3 ? 5 : 3)); // VTK_TRIANGLE, VTK_LINE
   std::vector<int32_t> zn(NC), rnk(NC, (int32_t)rank);
   for (size_t i = 0; i < NP; i++) { conn[i] = (int64_t)i; }
   for (size_t q = 0; q < NC; q++)
   {
      offs[q] = (int64_t)((q + 1) * dim);
      zn[q] = zone[q];
   }
   const int32_t cyc = cycle;
   auto ptr = [&](const double *q) { return q ? q : &none; };
   Appended ap;
   std::ostringstream h;
   h << "<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
        "header_type=\"UInt64\">\n<UnstructuredGrid>\n<FieldData>\n";
   h << ap.Array("Float64", "TIME", 0, &time, sizeof(double), " NumberOfTuples=\"1\"");
   h << ap.Array("Int32", "CYCLE", 0, &cyc, sizeof(int32_t), " NumberOfTuples=\"1\"");
   h << ap.Array("Float64", "ISO_VALUE", 0, &iso_value, sizeof(double), " NumberOfTuples=\"1\"");
   h << "</FieldData>\n<Piece NumberOfPoints=\"" << NP << "\" NumberOfCells=\"" << NC << "\">\n<Points>\n";
   h << ap.Array("Float64", "Points", 3, pts.data(), pts.size() * sizeof(double));
   h << "</Points>\n<Cells>\n";
   h << ap.Array("Int64", "connectivity", 0, conn.data(), conn.size() * sizeof(int64_t));
   h << ap.Array("Int64", "offsets", 0, offs.data(), offs.size() * sizeof(int64_t));
   h << ap.Array("UInt8", "types", 0, types.data(), types.size());
   h << "</Cells>\n<PointData Scalars=\"density\" Vectors=\"velocity\">\n";
   h << ap.Array("Float64", "density", 1, ptr(rho), NP * sizeof(double));
   h << ap.Array("Float64", "velocity", 3, vel.data(), vel.size() * sizeof(double));
   h << ap.Array("Float64", "specific_internal_energy", 1, ptr(e), NP * sizeof(double));
   h << ap.Array("Float64", "pressure", 1, ptr(p), NP * sizeof(double));
   for (const VtuField &f : extra) { h << ap.Array("Float64", f.name.c_str(), f.components, ptr(f.data), NP * f.components * sizeof(double)); }
   h << "</PointData>\n<CellData>\n";
   h << ap.Array("Int32", "zone", 1, zn.data(), zn.size() * sizeof(int32_t));
   h << ap.Array("Int32", "rank", 1, rnk.data(), rnk.size() * sizeof(int32_t));
   h << "</CellData>\n</Piece>\n</UnstructuredGrid>\n";
   MakeDirs(dir);
   std::ofstream f((dir + "/" + VtuName(cycle, nranks, rank)).c_str(), std::ios::binary);
   if (!f) { return false; }
   f << h.str();
   ap.Write(f);
   f << "</VTKFile>\n";
   f.close();
   return !f.fail();
}

// (the pieces of a contour dump carry the point and cell arrays of a volume dump: the .pvtu is the same)
bool WritePvtuContour(const std::string &dir, int cycle, double time, int nranks, const std::vector<VtuField> &extra)
{
   return WritePvtuFields(dir, cycle, time, nranks, extra);
}

bool WritePvd(const std::string &pvd_path, const std::string &rel_dir, const std::vector<double> &times,
              const std::vector<int> &cycles, int nranks)
{
   if (times.size() != cycles.size()) { return false; }
   const size_t slash = pvd_path.find_last_of('/');
   if (slash != std::string::npos) { MakeDirs(pvd_path.substr(0, slash)); }
   std::ofstream f(pvd_path.c_str());
   if (!f) { return false; }
   f << std::setprecision(17);
   f << "<?xml version=\"1.0\"?>\n<VTKFile type=\"Collection\" version=\"0.1\" byte_order=\"LittleEndian\">\n<Collection>\n";
   for (size_t i = 0; i < times.size(); i++)
   {
      f << "<DataSet timestep=\"" << times[i] << "\" group=\"\" part=\"0\" file=\"" << rel_dir << "/"
        << (nranks > 1 ? PvtuName(cycles[i]) : VtuName(cycles[i], 1, 0)) << "\"/>\n";
   }
   f << "</Collection>\n</VTKFile>\n";
   f.close();
   return !f.fail();
}

} // namespace laghos
