// scene_compile.cpp — scene compilation (scene_compile.h): validation, digest, BBox tree, the flattened
// trees and device tables, and the placement plan.  Pure host C++: no HIP, and the environment is read by
// tuning_from_env alone.
#include "scene_compile.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace rt {

namespace {
int fail(std::string* err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return code;
}
}  // namespace

SceneTuning tuning_from_env() {
  SceneTuning t;
  if (const char* e = getenv("SHIRLEY_COLLAPSE_DP")) t.collapse_dp = atoi(e) != 0;
  if (const char* e = getenv("SHIRLEY_LDS_NODES")) {
    t.has_lds_nodes = true;
    t.lds_nodes = atoll(e);
  }
  t.no_wide = getenv("SHIRLEY_NO_WIDE") != nullptr;
  t.no_lds_prims = getenv("SHIRLEY_NO_LDS_PRIMS") != nullptr;
  t.no_lds_mats = getenv("SHIRLEY_NO_LDS_MATS") != nullptr;
  t.no_lds_perlin = getenv("SHIRLEY_NO_LDS_PERLIN") != nullptr;
  t.no_hop = getenv("SHIRLEY_NO_HOP") != nullptr;
  if (const char* e = getenv("SHIRLEY_HOP")) {
    t.hop_root = std::strcmp(e, "root") == 0;
    t.hop_up = std::strcmp(e, "up") == 0;
    t.hop_general = std::strcmp(e, "general") == 0;
  }
  if (const char* e = getenv("SHIRLEY_SAH_BOXW")) t.sah_box_weight = atof(e);
  t.sah_binned = getenv("SHIRLEY_SAH_BINNED") != nullptr;
  t.wf_extend2 = getenv("SHIRLEY_WF_EXTEND2") != nullptr;
  if (const char* e = getenv("SHIRLEY_SPLIT_NT")) t.split_nt = atoi(e);
  if (const char* e = getenv("SHIRLEY_SPLIT_REFILL")) t.split_refill = std::max(1, atoi(e));
  return t;
}

// Book-2 extension parameters of an object, shared by the bounding box and the
// device record: RotateY's cos / sin (rotate_y.h: radians = degrees * pi / 180).
bool is_extended(const rt_object& o) {
  return o.geometry == RT_GEOM_MOVING_SPHERE || o.medium != 0 || o.transform != 0;
}
void rotate_y_cs(const rt_object& o, double& cs, double& sn) {
  const double rad = o.rotate_y_deg * 3.14159265358979323846 / 180.0;
  cs = std::cos(rad);
  sn = std::sin(rad);
}
// Does texture `ti` (a tree: children are earlier textures, validate()) read the hit's u, v?  Only an
// image leaf does (image_texture.rs:34-56); checker and marble read the point, solid nothing.
bool texture_uses_uv(const rt_scene_desc* d, int32_t ti) {
  if (ti < 0 || ti >= d->n_textures) return false;
  const rt_texture& t = d->textures[ti];
  if (t.kind == RT_TEX_IMAGE) return true;
  if (t.kind == RT_TEX_CHECKER) return texture_uses_uv(d, t.odd) || texture_uses_uv(d, t.even);
  return false;
}
// Book-2: Translate(RotateY(sphere)) of a plain sphere is the sphere about the moved centre — flattened
// into a world-space sphere before the tree is built, by the formula that maps an instance's hit point
// back to the world, so the instances take the reference sphere path (sphere leaf loop, no per-leaf ray
// transform).  t, point and normal agree with per-ray instancing in real arithmetic; u, v do not under a
// rotation (the instance's u is taken in its own frame, shifted by angle / 360), so a rotated sphere is
// flattened only when its material never reads u, v; rt_scene_hit then derives the instance's u, v from
// the record (uv_fixups).  The oracle flattens by the same rule (oracle.c flatten_instanced_sphere).
// DESIGN.md §10.
bool flattens(const rt_scene_desc* d, const rt_object& o) {
  if (o.geometry != RT_GEOM_SPHERE || !o.transform || o.medium) return false;
  if (o.rotate_y_deg == 0.0) return true;
  return o.material >= 0 && o.material < d->n_materials && !texture_uses_uv(d, d->materials[o.material].texture);
}
rt_object flat_object(const rt_scene_desc* d, const rt_object& o) {
  rt_object f = o;
  if (!flattens(d, o)) return f;
  double cs, sn;
  rotate_y_cs(o, cs, sn);
  const double cx = o.p[0], cy = o.p[1], cz = o.p[2];
  f.p[0] = (cs * cx + sn * cz) + o.offset[0];
  f.p[1] = cy + o.offset[1];
  f.p[2] = (-sn * cx + cs * cz) + o.offset[2];
  f.transform = 0;
  f.rotate_y_deg = 0.0;
  f.offset[0] = f.offset[1] = f.offset[2] = 0.0;
  return f;
}
// A scene description whose objects are flat_object's (the objects live in `store`).
rt_scene_desc flat_scene(const rt_scene_desc* d, std::vector<rt_object>& store) {
  store.resize((size_t)std::max(0, d->n_objects));
  for (int i = 0; i < d->n_objects; ++i) store[i] = flat_object(d, d->objects[i]);
  rt_scene_desc f = *d;
  f.objects = store.data();
  return f;
}
// A flattened rotated sphere's u, v as its instance reports them (sphere.rs:17-26 on the object-frame
// outward normal): the world normal rotated back by RotateY's inverse (rotate_y.h).
void instance_sphere_uv(double cs, double sn, rt_hit& h) {
  const double s = h.front_face ? 1.0 : -1.0;
  const double nx = s * h.normal[0], ny = s * h.normal[1], nz = s * h.normal[2];
  const double ox = cs * nx - sn * nz, oz = sn * nx + cs * nz;
  const double pi = 3.14159265358979323846;
  h.u = (std::atan2(-oz, ox) + pi) / (2.0 * pi);
  h.v = std::acos(-ny) / pi;
}
// moving_sphere.h center(time), the device's formula (the bounding box uses it at time0 and time1)
void moving_center(const rt_object& o, double tm, double* c) {
  const double s = (tm - o.q[3]) / (o.q[4] - o.q[3]);
  for (int k = 0; k < 3; ++k) c[k] = o.p[k] + (o.q[k] - o.p[k]) * s;
}

Box reference_box(const rt_object& o);
// object -> leaf box: the reference's bounding_box for reference objects; for book-2 objects the
// book's: moving_sphere.h (union of the boxes at time0 and time1), rotate_y.h (the 8 rotated
// corners), translate (box + offset), constant_medium.h (the boundary's box).
Box object_box(const rt_object& o) {
  if (!is_extended(o)) return reference_box(o);
  Box b{};
  if (o.geometry == RT_GEOM_MOVING_SPHERE) {
    double c0[3], c1[3];
    moving_center(o, o.q[3], c0);
    moving_center(o, o.q[4], c1);
    Box b0{}, b1{};
    for (int k = 0; k < 3; ++k) {
      b0.mn[k] = c0[k] - o.p[3];
      b0.mx[k] = c0[k] + o.p[3];
      b1.mn[k] = c1[k] - o.p[3];
      b1.mx[k] = c1[k] + o.p[3];
    }
    b = surrounding(b0, b1);
  } else {
    b = reference_box(o);
  }
  if (o.transform) {
    double cs, sn;
    rotate_y_cs(o, cs, sn);
    Box r{};
    for (int k = 0; k < 3; ++k) {
      r.mn[k] = std::numeric_limits<double>::infinity();
      r.mx[k] = -std::numeric_limits<double>::infinity();
    }
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        for (int k = 0; k < 2; ++k) {
          const double x = i * b.mx[0] + (1 - i) * b.mn[0];
          const double y = j * b.mx[1] + (1 - j) * b.mn[1];
          const double z = k * b.mx[2] + (1 - k) * b.mn[2];
          const double nx = cs * x + sn * z, nz = -sn * x + cs * z;
          const double t[3] = {nx, y, nz};
          for (int c = 0; c < 3; ++c) {
            r.mn[c] = std::fmin(r.mn[c], t[c]);
            r.mx[c] = std::fmax(r.mx[c], t[c]);
          }
        }
    for (int k = 0; k < 3; ++k) {
      r.mn[k] += o.offset[k];
      r.mx[k] += o.offset[k];
    }
    b = r;
  }
  return b;
}

// exactly the reference's bounding_box (sphere.rs:54-60, rect.rs:82-99, rect.rs:158-163)
Box reference_box(const rt_object& o) {
  Box b{};
  if (o.geometry == RT_GEOM_SPHERE) {
    for (int k = 0; k < 3; ++k) {
      b.mn[k] = o.p[k] - o.p[3];
      b.mx[k] = o.p[k] + o.p[3];
    }
  } else if (o.geometry == RT_GEOM_RECT_BOX) {
    for (int k = 0; k < 3; ++k) {
      b.mn[k] = o.p[k];
      b.mx[k] = o.p[k + 3];
    }
  } else {
    int D1 = (o.geometry == RT_GEOM_RECT_YZ) ? 1 : 0;
    int D2 = (o.geometry == RT_GEOM_RECT_XY) ? 1 : 2;
    int n = 3 - D1 - D2;
    b.mn[D1] = o.p[0];
    b.mx[D1] = o.p[1];
    b.mn[D2] = o.p[2];
    b.mx[D2] = o.p[3];
    b.mn[n] = o.p[4] - 0.0001;  // BBOX_WIDTH, rect.rs:9
    b.mx[n] = o.p[4] + 0.0001;
  }
  return b;
}

int validate(const rt_scene_desc* d, std::string* err) {
  if (!d) return fail(err, RT_E_INVALID, "scene is NULL");
  if (d->n_objects < 0 || d->n_materials < 0 || d->n_textures < 0 || d->n_perlin < 0 || d->n_images < 0)
    return fail(err, RT_E_INVALID, "negative count in scene");
  if ((d->n_objects && !d->objects) || (d->n_materials && !d->materials) || (d->n_textures && !d->textures) ||
      (d->n_perlin && !d->perlin) || (d->n_images && !d->images))
    return fail(err, RT_E_INVALID, "NULL array with non-zero count");
  if (d->sky < RT_SKY_ABOVE || d->sky > RT_SKY_NONE) return fail(err, RT_E_INVALID, "bad skybox %d", d->sky);
  for (int i = 0; i < d->n_objects; ++i) {
    const rt_object& o = d->objects[i];
    if (o.geometry < RT_GEOM_SPHERE || o.geometry > RT_GEOM_MOVING_SPHERE)
      return fail(err, RT_E_INVALID, "object %d: bad geometry %d", i, o.geometry);
    if ((o.medium != 0 && o.medium != 1) || (o.transform != 0 && o.transform != 1))
      return fail(err, RT_E_INVALID, "object %d: medium / transform flags must be 0 or 1", i);
    if (o.geometry == RT_GEOM_MOVING_SPHERE && !(o.q[4] != o.q[3]))
      return fail(err, RT_E_INVALID, "object %d: moving sphere needs time0 != time1", i);
    if (o.medium && (o.material < 0 || o.material >= d->n_materials || d->materials[o.material].kind != RT_MAT_ISOTROPIC))
      return fail(err, RT_E_INVALID, "object %d: a constant medium takes an isotropic material", i);
    if (o.material < 0 || o.material >= d->n_materials)
      return fail(err, RT_E_INVALID, "object %d: material %d out of range", i, o.material);
  }
  for (int i = 0; i < d->n_materials; ++i) {
    const rt_material& m = d->materials[i];
    if (m.kind < RT_MAT_METAL || m.kind > RT_MAT_ISOTROPIC)
      return fail(err, RT_E_INVALID, "material %d: bad kind %d", i, m.kind);
    bool textured = m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_DIFFUSE_LIGHT || m.kind == RT_MAT_FAIRY_LIGHT ||
                    m.kind == RT_MAT_ISOTROPIC;
    if (textured && (m.texture < 0 || m.texture >= d->n_textures))
      return fail(err, RT_E_INVALID, "material %d: texture %d out of range", i, m.texture);
  }
  for (int i = 0; i < d->n_textures; ++i) {
    const rt_texture& t = d->textures[i];
    switch (t.kind) {
      case RT_TEX_SOLID: break;
      case RT_TEX_CHECKER:
        if (t.odd < 0 || t.odd >= d->n_textures || t.even < 0 || t.even >= d->n_textures)
          return fail(err, RT_E_INVALID, "texture %d: checker child out of range", i);
        // children must be earlier textures: guarantees the lookup terminates (no cycles)
        if (t.odd >= i || t.even >= i) return fail(err, RT_E_INVALID, "texture %d: checker children must precede it", i);
        break;
      case RT_TEX_PERLIN:
        if (t.table < 0 || t.table >= d->n_perlin) return fail(err, RT_E_INVALID, "texture %d: perlin table", i);
        break;
      case RT_TEX_IMAGE:
        if (t.table < 0 || t.table >= d->n_images) return fail(err, RT_E_INVALID, "texture %d: image index", i);
        break;
      default: return fail(err, RT_E_INVALID, "texture %d: bad kind %d", i, t.kind);
    }
  }
  for (int i = 0; i < d->n_perlin; ++i)
    for (int k = 0; k < 256; ++k) {
      const rt_perlin_table& T = d->perlin[i];
      if (T.perm_x[k] < 0 || T.perm_x[k] > 255 || T.perm_y[k] < 0 || T.perm_y[k] > 255 || T.perm_z[k] < 0 ||
          T.perm_z[k] > 255)
        return fail(err, RT_E_INVALID, "perlin table %d: permutation entry out of [0,255]", i);
    }
  for (int i = 0; i < d->n_images; ++i)
    if (d->images[i].width < 1 || d->images[i].height < 1 || !d->images[i].rgb)
      return fail(err, RT_E_INVALID, "image %d: empty", i);
  return RT_OK;
}

uint64_t scene_digest(const rt_scene_desc* d, int32_t builder) {
  Fnv1a f;
  f.val(builder);
  f.val(d->sky);
  f.bytes(d->sky_color, sizeof d->sky_color);
  f.val(d->n_objects);
  for (int i = 0; i < d->n_objects; ++i) {
    const rt_object& o = d->objects[i];
    f.val(o.geometry); f.val(o.material); f.bytes(o.p, sizeof o.p); f.val(o.medium); f.val(o.transform);
    f.bytes(o.q, sizeof o.q); f.val(o.density); f.val(o.rotate_y_deg); f.bytes(o.offset, sizeof o.offset);
  }
  f.val(d->n_materials);
  for (int i = 0; i < d->n_materials; ++i) {
    const rt_material& m = d->materials[i];
    f.val(m.kind); f.val(m.texture); f.bytes(m.albedo, sizeof m.albedo); f.val(m.param);
  }
  f.val(d->n_textures);
  for (int i = 0; i < d->n_textures; ++i) {
    const rt_texture& t = d->textures[i];
    f.val(t.kind); f.val(t.odd); f.val(t.even); f.val(t.table); f.bytes(t.color, sizeof t.color); f.val(t.scale);
  }
  f.val(d->n_perlin);
  for (int i = 0; i < d->n_perlin; ++i) {
    const rt_perlin_table& t = d->perlin[i];
    f.bytes(t.ranfloat, sizeof t.ranfloat); f.bytes(t.perm_x, sizeof t.perm_x); f.bytes(t.perm_y, sizeof t.perm_y);
    f.bytes(t.perm_z, sizeof t.perm_z);
  }
  f.val(d->n_images);
  for (int i = 0; i < d->n_images; ++i) {
    const rt_image& m = d->images[i];
    f.val(m.width); f.val(m.height);
    f.bytes(m.rgb, (size_t)m.width * m.height * 3);
  }
  return f.h;
}

// Leaf order of a tree, lhs before rhs (in-order): rank[object]; objects outside it (a SAH tree leaves out
// the never-hit inverted boxes) follow in index order.
std::vector<int32_t> reference_ranks(const BuiltTree& t, int32_t n) {
  std::vector<int32_t> rank((size_t)std::max(0, n), -1);
  int32_t next = 0;
  if (t.root >= 0) {
    std::vector<int32_t> stack{t.root};
    while (!stack.empty()) {
      const BuildNode& nd = t.nodes[stack.back()];
      stack.pop_back();
      if (nd.leaf >= 0) {
        if (rank[nd.leaf] < 0) rank[nd.leaf] = next++;
        continue;
      }
      stack.push_back(nd.rhs);  // (popped after the whole lhs subtree)
      stack.push_back(nd.lhs);
    }
  }
  for (int32_t i = 0; i < n; ++i)
    if (rank[i] < 0) rank[i] = next++;
  return rank;
}

BuiltTree build_tree(const rt_scene_desc* d, int32_t builder, const SceneTuning& tune) {
  std::vector<Box> boxes(d->n_objects);
  for (int i = 0; i < d->n_objects; ++i) boxes[i] = object_box(d->objects[i]);
  // The sweep's split cost weighs a RectBox leaf (six faces, the costliest exact test) 4, every other
  // object 1: Cornell +5.4 %, headline ±0.  SHIRLEY_SAH_BOXW=<c>: the weight (tuning; 1 = the
  // plain count).  Scenes without a RectBox build the unweighted tree.
  std::vector<double> w;
  const double box_weight = tune.sah_box_weight;
  bool any_box = false;
  for (int i = 0; i < d->n_objects; ++i) any_box = any_box || d->objects[i].geometry == RT_GEOM_RECT_BOX;
  if (any_box && box_weight != 1.0) {
    w.assign(d->n_objects, 1.0);
    for (int i = 0; i < d->n_objects; ++i)
      if (d->objects[i].geometry == RT_GEOM_RECT_BOX) w[i] = box_weight;
  }
  return builder == RT_BVH_SAH ? build_sah_tree(boxes, !tune.sah_binned, w.empty() ? nullptr : &w)
                               : build_reference_tree(boxes);
}

void box_to6(const Box& b, double* o) {
  for (int k = 0; k < 3; ++k) {
    o[k] = b.mn[k];
    o[k + 3] = b.mx[k];
  }
}

// BuiltTree -> DNode array in breadth-first order (node 0 = top node whose child 0 is the root), so
// that a prefix of the array = the top levels of the tree, which the kernels keep in LDS.
void flatten(const BuiltTree& t, std::vector<DNode>& out) {
  out.clear();
  DNode top{};
  top.child[0] = kEmptyChild;
  top.child[1] = kEmptyChild;
  out.push_back(top);
  if (t.root < 0) return;
  struct Item {
    int32_t built;
    int32_t parent;
    int slot;
  };
  std::vector<Item> q{{t.root, 0, 0}};
  for (size_t head = 0; head < q.size(); ++head) {
    Item it = q[head];
    const BuildNode& bn = t.nodes[it.built];
    box_to6(bn.box, out[it.parent].box[it.slot]);
    if (bn.leaf >= 0) {
      out[it.parent].child[it.slot] = ~bn.leaf;
      continue;
    }
    int32_t idx = (int32_t)out.size();
    out[it.parent].child[it.slot] = idx;
    out.push_back(DNode{});
    q.push_back({bn.lhs, idx, 0});
    q.push_back({bn.rhs, idx, 1});
  }
}

// Collapse heuristic: half the surface area of a box (0 for an inverted or NaN box).
double half_area(const Box& b) {
  const double x = b.mx[0] - b.mn[0], y = b.mx[1] - b.mn[1], z = b.mx[2] - b.mn[2];
  if (!(x >= 0.0 && y >= 0.0 && z >= 0.0)) return 0.0;
  return x * y + y * z + z * x;
}

// BuiltTree -> 4-wide nodes for the megakernel: each node takes its two children and then, while
// it has fewer than four, replaces its largest-area internal child by that child's two children
// (order kept).  Boxes stay the reference's exact boxes.  `stack_bound` = the worst-case traversal
// stack: the sum over a root path of (internal children - 1) per node (at most that many pushes).
// f32 bounds rounded outward (f32 cast rounds to nearest; step once more if it landed inside).
float round_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = std::nextafter(f, -INFINITY);
  return f;
}
float round_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafter(f, INFINITY);
  return f;
}

// Node-box inflation and the ray-origin range it covers.  The f32 node test computes
// t = fma(plane, 1/d, -o*(1/d)) from o and 1/d rounded to f32: in space units its error is at most
// ~2^-22 (|o| + |plane|); inflating every stored box by delta = 2^-20 (L + B) (B = largest finite
// |plane|) and rounding outward keeps the test a superset of the exact one for every ray with
// max|o| <= L, with a 4x margin.
struct Inflation {
  double delta;
  float origin_limit;
  double box_bound;  // B: the largest finite |plane| of any box
};
Inflation inflation_for(const BuiltTree& t) {
  double B = 0.0;
  for (const BuildNode& n : t.nodes)
    for (int k = 0; k < 3; ++k) {
      if (std::isfinite(n.box.mn[k])) B = std::max(B, std::fabs(n.box.mn[k]));
      if (std::isfinite(n.box.mx[k])) B = std::max(B, std::fabs(n.box.mx[k]));
    }
  const double L = std::max(16.0, 4.0 * B);
  return Inflation{std::ldexp(L + B, -20), (float)L, B};
}

// child slot of a 4-wide node: an empty slot never passes (lo = +inf > hi = -inf); a box with a
// NaN plane always passes (its leaf is tested exactly anyway)
void set_child_box(DNode4F& n, int slot, const Box* b, double delta) {
  for (int a = 0; a < 3; ++a) {
    float lo, hi;
    if (!b) {
      lo = INFINITY;
      hi = -INFINITY;
    } else if (std::isnan(b->mn[a]) || std::isnan(b->mx[a])) {
      lo = -INFINITY;
      hi = INFINITY;
    } else {
      lo = round_down(b->mn[a] - delta);
      hi = round_up(b->mx[a] + delta);
    }
    n.row[a][0][slot] = lo;
    n.row[a][1][slot] = hi;
    n.row[a][2][slot] = lo;
  }
}

// Optimal collapse of the binary tree into 4-wide nodes: minimises the sum of the surface areas of
// the 4-wide internal nodes (expected node visits of a ray, SAH), by dynamic programming over the
// binary tree.  H(n, j) = least cost of covering subtree n with at most j child slots of its
// parent: one slot holds n itself (a leaf: cost 0; an internal node: its own 4-wide node,
// F(n) = area(n) + G(n, 4)), more slots may open n into its two children, G(n, k) = min over the
// split j of H(lhs, j) + H(rhs, k - j).  Leaf costs do not depend on the collapse (every object is
// one child slot) and are left out.
struct Collapse4 {
  const BuiltTree* t = nullptr;
  std::vector<double> H, G;    // [n * 5 + j], j = 1..4
  std::vector<int8_t> split;   // argmin j of G(n, k), [n * 5 + k]
  bool ready() const { return t != nullptr; }
  void build(const BuiltTree& tree) {
    t = &tree;
    const size_t nn = tree.nodes.size();
    H.assign(nn * 5, 0.0);
    G.assign(nn * 5, INFINITY);
    split.assign(nn * 5, 1);
    // children come before parents in neither builder's order for sure: iterative post-order
    std::vector<std::pair<int32_t, bool>> st{{tree.root, false}};
    while (!st.empty()) {
      auto [n, done] = st.back();
      st.pop_back();
      const BuildNode& b = tree.nodes[n];
      if (b.leaf >= 0) continue;  // H = 0
      if (!done) {
        st.push_back({n, true});
        st.push_back({b.lhs, false});
        st.push_back({b.rhs, false});
        continue;
      }
      for (int k = 2; k <= 4; ++k)
        for (int j = 1; j < k; ++j) {
          const double c = H[b.lhs * 5 + j] + H[b.rhs * 5 + (k - j)];
          if (c < G[n * 5 + k]) { G[n * 5 + k] = c; split[n * 5 + k] = (int8_t)j; }
        }
      const double f = half_area(b.box) + G[n * 5 + 4];
      H[n * 5 + 1] = f;
      for (int j = 2; j <= 4; ++j) H[n * 5 + j] = std::min(f, G[n * 5 + j]);
    }
  }
  // the child slots of the 4-wide node made from internal binary node n
  void children(int32_t n, std::vector<int32_t>& out) const {
    out.clear();
    collect(t->nodes[n].lhs, split[n * 5 + 4], out);
    collect(t->nodes[n].rhs, 4 - split[n * 5 + 4], out);
  }
  void collect(int32_t c, int j, std::vector<int32_t>& out) const {
    const BuildNode& b = t->nodes[c];
    if (b.leaf >= 0 || j == 1 || !(G[c * 5 + j] < H[c * 5 + 1])) {
      out.push_back(c);
      return;
    }
    collect(b.lhs, split[c * 5 + j], out);
    collect(b.rhs, j - split[c * 5 + j], out);
  }
};

// use_dp: the optimal collapse (Collapse4) instead of the greedy one (open the largest-area internal
// child until four slots are filled).  rt_scene_upload picks it for the scenes the megakernel runs with
// the whole scene in LDS, greedy for the rest.
void flatten4(const BuiltTree& t, const rt_scene_desc* d, double delta, std::vector<DNode4F>& out,
              int32_t& stack_bound, bool use_dp) {
  Collapse4 dp;
  if (t.root >= 0 && use_dp) dp.build(t);
  out.clear();
  DNode4F top{};
  for (int k = 0; k < 4; ++k) {
    top.child[k] = kEmptyChild;
    set_child_box(top, k, nullptr, delta);
  }
  out.push_back(top);
  stack_bound = 1;
  if (t.root < 0) return;
  auto internal = [&](int32_t n) { return t.nodes[n].leaf < 0; };
  struct Item {
    int32_t built;
    int32_t parent;
    int slot;
    int32_t level;  // stack entries that can be live when this node is visited
  };
  std::vector<Item> q{{t.root, 0, 0, 0}};
  for (size_t head = 0; head < q.size(); ++head) {
    const Item it = q[head];
    const BuildNode& bn = t.nodes[it.built];
    set_child_box(out[it.parent], it.slot, &bn.box, delta);
    if (bn.leaf >= 0) {
      const int32_t g = d->objects[bn.leaf].geometry;
      // book-2 objects take the "box" (slow) leaf loop, which dispatches on the primitive
      const int32_t flags = is_extended(d->objects[bn.leaf]) ? kLeafGeneric | kLeafBox
                            : g == RT_GEOM_SPHERE            ? 0
                            : (g == RT_GEOM_RECT_BOX ? kLeafGeneric | kLeafBox : kLeafGeneric);
      out[it.parent].child[it.slot] = ~(bn.leaf | flags);
      continue;
    }
    const int32_t idx = (int32_t)out.size();
    out[it.parent].child[it.slot] = idx;
    DNode4F nd{};
    for (int k = 0; k < 4; ++k) {
      nd.child[k] = kEmptyChild;
      set_child_box(nd, k, nullptr, delta);
    }
    out.push_back(nd);
    std::vector<int32_t> ch;
    if (dp.ready()) {
      dp.children(it.built, ch);
    } else {
      ch = {bn.lhs, bn.rhs};
      while (ch.size() < 4) {
        int pick = -1;
        double best = -1.0;
        for (size_t i = 0; i < ch.size(); ++i)
          if (internal(ch[i]) && half_area(t.nodes[ch[i]].box) > best) {
            best = half_area(t.nodes[ch[i]].box);
            pick = (int)i;
          }
        if (pick < 0) break;
        const int32_t x = ch[pick];
        ch[pick] = t.nodes[x].lhs;
        ch.insert(ch.begin() + pick + 1, t.nodes[x].rhs);
      }
    }
    int n_int = 0;
    for (int32_t c : ch) n_int += internal(c) ? 1 : 0;
    const int32_t level = it.level + std::max(0, n_int - 1);
    stack_bound = std::max(stack_bound, level + 1);
    for (size_t i = 0; i < ch.size(); ++i) q.push_back({ch[i], idx, (int)i, level});
  }
}
namespace {

// The ground stack of a compiled scene (rt_layout.h DGround; the proof: DESIGN.md §3.1), or false when the
// scene has none and the hop pass keeps its first-node visit.  G = the rects and RectBoxes; every test below is
// an exact binary64 comparison of the values the reference's own leaf boxes hold (rt_device.h leaf_box).
//   * 1 <= |G| <= kGroundMaxPrims, every rect of G an XZ rect, every other primitive a plain sphere, r > 0
//     (or one the reference never hits, sphere_never_hit);
//   * Y = the largest hi_y of G's leaf boxes; every sphere's box starts at c.y - r >= Y;
//   * every y plane of G is Y itself or at least `gap` below it;
//   * the bounds the proof's constants assume: coordinates <= 2^20, radii <= 2^10, eta <= 2^-16, m <= 2^-13;
//   * the guard bitmap has at most kGroundMaxCells cells.
// Constants (names as in the proof): R = 2^10 the largest |d_xz| / |d.y| of a served ray; reach = the slab's
// thickness times R + 1, the longest served segment; L^2 = (D + reach)^2 + reach^2 + r_max^2 with D the largest
// distance from a point of G's extent to a sphere centre; m = 2^-38 L^2, 2^10 times the residual bound
// 32 * 2^-53 L^2 of a root the reference's sphere test computes; eta = m / (2 r_min), the depth below a sphere's
// lowest point from which |p - c|^2 - r^2 > m; tol = 2^-40 max(1, |Y|, |lowest plane|).
// A sphere of radius <= 0 whose leaf box c -+ r (sphere.rs:54-60) is inverted or flat along y: hit2 (aabb.rs:62-79)
// ends with t1 <= t0 on that axis for every ray with a finite non-zero d.y, so the reference never tests the
// sphere for such a ray (random_scene holds two: check_fit_ball shrinks a ball below zero where it overlaps).
bool sphere_never_hit(const double* p) { return p[3] <= 0.0 && p[1] - p[3] >= p[1] + p[3]; }
// (the proof's constants that plane_stack below builds on: gap, tol, reach and B, the largest |x|, |z| of G's extent)
struct GroundConsts {
  double gap = 0.0, tol = 0.0, reach = 0.0, ext = 0.0;
  double sph_top = 0.0;  // the highest plane of a sphere's leaf box (Y when the scene holds no sphere)
};
bool ground_stack(const std::vector<DPrim>& prims, int n_prims, std::vector<uint32_t>& out, GroundConsts* consts = nullptr) {
  out.clear();
  std::vector<int32_t> boxes, rects;
  double top = -std::numeric_limits<double>::infinity(), low = -top;
  double ex0 = low, ex1 = top, ez0 = low, ez1 = top, r_min = low, r_max = 0.0;
  std::vector<double> planes;
  for (int i = 0; i < n_prims; ++i) {
    const DPrim& q = prims[i];
    const double* p = q.p;
    if (q.kind == kPrimBox) {
      boxes.push_back(i);
      planes.push_back(p[1]);
      planes.push_back(p[4]);
      top = std::max(top, p[4]);
      ex0 = std::min(ex0, p[0]), ex1 = std::max(ex1, p[3]), ez0 = std::min(ez0, p[2]), ez1 = std::max(ez1, p[5]);
    } else if (q.kind == kPrimRectXZ) {
      rects.push_back(i);
      planes.push_back(p[4]);
      top = std::max(top, p[4] + 0.0001);  // (leaf_box: the rect's box is padded along its normal)
      ex0 = std::min(ex0, p[0]), ex1 = std::max(ex1, p[1]), ez0 = std::min(ez0, p[2]), ez1 = std::max(ez1, p[3]);
    } else if (q.kind == kPrimSphere) {
      if (!std::isfinite(p[3])) return false;
      if (sphere_never_hit(p)) continue;
      if (!(p[3] > 0.0)) return false;
      r_min = std::min(r_min, p[3]);
      r_max = std::max(r_max, p[3]);
    } else {
      return false;  // another rect orientation, a moving sphere, an extended primitive
    }
  }
  const size_t n_g = boxes.size() + rects.size();
  if (n_g < 1 || n_g > (size_t)kGroundMaxPrims) return false;
  for (double y : planes) low = std::min(low, y);
  const double big = 0x1p20;
  if (!(std::fabs(top) <= big && std::fabs(low) <= big && ex0 >= -big && ex1 <= big && ez0 >= -big && ez1 <= big &&
        ex0 <= ex1 && ez0 <= ez1 && r_max <= 0x1p10))
    return false;
  double dist = 0.0;  // D
  std::vector<const DPrim*> guarded;
  for (int i = 0; i < n_prims; ++i) {
    const DPrim& q = prims[i];
    if (q.kind != kPrimSphere || sphere_never_hit(q.p)) continue;
    const double* p = q.p;
    const double lo_y = p[1] - p[3];  // the sphere's leaf box (leaf_box), rounded as the reference rounds it
    if (!(lo_y >= top) || !(std::fabs(p[0]) <= big && std::fabs(p[1]) <= big && std::fabs(p[2]) <= big)) return false;
    const double dx = std::max(std::fabs(p[0] - ex0), std::fabs(p[0] - ex1));
    const double dy = std::max(std::fabs(p[1] - low), std::fabs(p[1] - top));
    const double dz = std::max(std::fabs(p[2] - ez0), std::fabs(p[2] - ez1));
    dist = std::max(dist, std::sqrt(dx * dx + dy * dy + dz * dz));
    if (lo_y - top < kGroundGuard / 2) guarded.push_back(&q);  // (one floating higher needs no guard: §3.1)
  }
  const double ratio = 0x1p10, tol = 0x1p-40 * std::max(1.0, std::max(std::fabs(top), std::fabs(low)));
  const double reach = ((top - low) + 2.0 * tol) * (ratio + 1.0);
  const double l2 = (dist + reach) * (dist + reach) + reach * reach + r_max * r_max;
  const double m = 0x1p-38 * l2;
  const double eta = std::isfinite(r_min) ? m / (2.0 * r_min) : 0.0;
  // (eta <= the guard radius / (2 R), far below the 1/64 of a floating sphere; m <= half of (guard radius / 2)^2)
  if (!(eta <= 0x1p-16 && m <= 0x1p-13)) return false;
  const double gap = 4.0 * eta + 4.0 * tol;
  for (double y : planes)
    if (y != top && !(y <= top - gap)) return false;
  if (consts) {
    consts->gap = gap;
    consts->tol = tol;
    consts->reach = reach;
    consts->ext = std::max(std::max(std::fabs(ex0), std::fabs(ex1)), std::max(std::fabs(ez0), std::fabs(ez1)));
    consts->sph_top = top;
    for (int i = 0; i < n_prims; ++i)
      if (prims[i].kind == kPrimSphere && !sphere_never_hit(prims[i].p))
        consts->sph_top = std::max(consts->sph_top, prims[i].p[1] + prims[i].p[3]);
  }

  DGround g;
  std::memset(&g, 0, sizeof g);
  g.y_lo = low - tol;
  g.y_hi = top + tol;
  g.y_top = top;
  g.dy_min = std::max((2.0 * eta + 4.0 * tol) / 0.001, 0x1p-100);  // / the renderer's t_min (render.rs:30)
  g.y_down = top - gap;
  g.ratio2 = ratio * ratio;
  g.n = (int32_t)n_g;
  g.n_box = (int32_t)boxes.size();
  for (size_t i = 0; i < boxes.size(); ++i) g.prim[i] = boxes[i];
  for (size_t i = 0; i < rects.size(); ++i) g.prim[boxes.size() + i] = rects[i];
  // the guard bitmap over the guarded contact points' rectangle, two cells of margin
  size_t words = 0;
  if (!guarded.empty()) {
    double cx0 = guarded[0]->p[0], cx1 = cx0, cz0 = guarded[0]->p[2], cz1 = cz0;
    for (const DPrim* q : guarded) {
      cx0 = std::min(cx0, q->p[0]), cx1 = std::max(cx1, q->p[0]);
      cz0 = std::min(cz0, q->p[2]), cz1 = std::max(cz1, q->p[2]);
    }
    g.x0 = std::floor(cx0 * kGroundCellsPerUnit - 2.0) * kGroundCell;
    g.z0 = std::floor(cz0 * kGroundCellsPerUnit - 2.0) * kGroundCell;
    const double nx = std::ceil((cx1 - g.x0) * kGroundCellsPerUnit + 2.0), nz = std::ceil((cz1 - g.z0) * kGroundCellsPerUnit + 2.0);
    if (!(nx * nz <= (double)kGroundMaxCells)) return false;
    g.nx = (int32_t)nx;
    g.nz = (int32_t)nz;
    words = ((size_t)g.nx * (size_t)g.nz + 31) / 32;
  }
  out.assign(sizeof(DGround) / 4 + words, 0u);
  std::memcpy(out.data(), &g, sizeof g);
  uint32_t* bits = out.data() + sizeof(DGround) / 4;
  // a cell is marked when some point of it lies within the guard radius (with 2^-20 of slack for the cell
  // index's rounding, ground_cell) of a guarded contact point
  const double rad = kGroundGuard * (1.0 + 0x1p-20);
  for (const DPrim* q : guarded) {
    const double cx = q->p[0], cz = q->p[2];
    const int i0 = ground_cell(cx, g.x0, g.nx), k0 = ground_cell(cz, g.z0, g.nz);  // (inside by the margin)
    const int span = (int)std::ceil(rad * kGroundCellsPerUnit) + 1;
    for (int k = std::max(0, k0 - span); k <= std::min(g.nz - 1, k0 + span); ++k)
      for (int i = std::max(0, i0 - span); i <= std::min(g.nx - 1, i0 + span); ++i) {
        const double x_lo = g.x0 + i * kGroundCell, z_lo = g.z0 + k * kGroundCell;
        const double dx = std::max(0.0, std::max(x_lo - cx, cx - (x_lo + kGroundCell)));
        const double dz = std::max(0.0, std::max(z_lo - cz, cz - (z_lo + kGroundCell)));
        if (dx * dx + dz * dz <= rad * rad) {
          const size_t c = (size_t)k * (size_t)g.nx + (size_t)i;
          bits[c >> 5] |= 1u << (c & 31);
        }
      }
  }
  return true;
}

// Is the ground stack `ground` (ground_stack's record) a plane stack (rt_layout.h DPlanes; the proof: DESIGN.md
// §3.1)?  Exact binary64 compares on the values the reference's leaf boxes hold, like ground_stack's:
//   * no two y planes of G — a rect's own plane, both faces of a RectBox — within `gap` of each other;
//   * the rectangle common to every primitive's xz extent, shrunk by mx on each side, is not empty and contains the
//     guard bitmap's rectangle.
// mx = 2^-44 (B + reach + 1): 2^4 times the 2^-48 (B + L) of sphere_t_sure's eta, with the longest served segment's
// horizontal run for L — far above the 3 * 2^-53 (B + reach) a hit point o + t d is off by, and above the
// 2^-50 (B + reach) that keeps a side plane's quotient and slab product strictly behind the hit's.
// The record's tail is plane_first's (the traversal's own rays, which may start up to H above Y): a second core, shrunk
// for that longer reach, Y + H, and the grown extent of "over the edge".  Whether a stack is a plane stack, and the hop
// passes' core, do not depend on it.
bool plane_stack(const std::vector<DPrim>& prims, const std::vector<DMat>& mats, const std::vector<uint32_t>& ground,
                 const GroundConsts& k, std::vector<uint32_t>& out) {
  out.clear();
  DGround g;
  std::memcpy(&g, ground.data(), sizeof g);
  const double inf = std::numeric_limits<double>::infinity();
  double x0 = -inf, x1 = inf, z0 = -inf, z1 = inf;
  struct Plane {
    double y;
    int32_t info;
  };
  std::vector<Plane> pl;
  // (the answers: rt_device.h kHopRefused 0, kHopServed 1, kHopFound 2; a rect counts by the top of its padded box
  // for y_down, as ground_hop_t does)
  auto info = [](int32_t prim, int face, int answer, bool top) {
    return (int32_t)((uint32_t)prim << 5 | (top ? 16u : 0u) | (uint32_t)answer << 2 | (face < 0 ? 0u : (face == 4 ? 1u : 2u)));
  };
  for (int i = 0; i < g.n; ++i) {
    const int32_t leaf = g.prim[i];
    if (leaf < 0 || leaf >= (1 << 26)) return false;
    const DPrim& q = prims[leaf];
    const double* p = q.p;
    const bool diel = mats[q.material].kind == RT_MAT_DIELECTRIC;
    if (i < g.n_box) {
      x0 = std::max(x0, p[0]), x1 = std::min(x1, p[3]), z0 = std::max(z0, p[2]), z1 = std::min(z1, p[5]);
      for (int face = 4; face <= 5; ++face) {
        const double y = face == 4 ? p[4] : p[1];
        pl.push_back({y, info(leaf, face, diel ? 1 : (y <= g.y_down ? 2 : 0), y == g.y_top)});
      }
    } else {
      x0 = std::max(x0, p[0]), x1 = std::min(x1, p[1]), z0 = std::max(z0, p[2]), z1 = std::min(z1, p[3]);
      pl.push_back({p[4], info(leaf, -1, (!diel && p[4] + 0.0001 <= g.y_down) ? 2 : 0, false)});
    }
  }
  std::stable_sort(pl.begin(), pl.end(), [](const Plane& a, const Plane& b) { return a.y < b.y; });
  for (size_t i = 1; i < pl.size(); ++i)
    if (!(pl[i].y - pl[i - 1].y > k.gap)) return false;
  const double mx = 0x1p-44 * (k.ext + k.reach + 1.0);
  DPlanes d;
  std::memset(&d, 0, sizeof d);
  d.x0 = x0 + mx, d.x1 = x1 - mx, d.z0 = z0 + mx, d.z1 = z1 - mx;
  if (!(d.x0 < d.x1 && d.z0 < d.z1)) return false;
  if (g.nx > 0 && !(g.x0 >= d.x0 && g.x0 + g.nx * kGroundCell <= d.x1 && g.z0 >= d.z0 && g.z0 + g.nz * kGroundCell <= d.z1))
    return false;
  d.tol = k.tol;
  d.n = (int32_t)pl.size();
  for (size_t i = 0; i < pl.size(); ++i) d.y[i] = pl[i].y, d.info[i] = pl[i].info;
  // plane_first (rt_device.h): the traversal's rays start up to H above Y — H covers every point of the sphere boxes
  // twice over, and at least 8 (random_scene's camera sits 2 above its ground) — so their longest segment runs
  // H (R + 1) further than a hop's, and their core is shrunk by the margin of that reach.  An empty core (fx0 > fx1)
  // makes every ray decline; the hop passes' core above is untouched.
  const double height = std::min(0x1p20, std::max(8.0, 2.0 * (k.sph_top - g.y_top)));
  const double reach_f = k.reach + height * (0x1p10 + 1.0);
  const double mxf = 0x1p-44 * (k.ext + reach_f + 1.0);
  d.fx0 = x0 + mxf, d.fx1 = x1 - mxf, d.fz0 = z0 + mxf, d.fz1 = z1 - mxf;
  if (!(d.fx0 < d.fx1 && d.fz0 < d.fz1)) d.fx0 = d.fz0 = inf, d.fx1 = d.fz1 = -inf;
  d.y_max = g.y_top + height;
  // ... and "over the edge": the rectangle that holds every primitive's xz extent, grown by mo = 2^-23 (B + reach + 1).
  // A crossing of the highest plane that far outside it puts every earlier side-plane crossing mo / R above that
  // plane, 2^10 times the rounding of a hit point's y at the largest coordinates ground_stack admits (§3.1)
  const double mo = 0x1p-23 * (k.ext + reach_f + 1.0);
  double ux0 = inf, ux1 = -inf, uz0 = inf, uz1 = -inf;
  for (int i = 0; i < g.n; ++i) {
    const double* p = prims[g.prim[i]].p;
    const bool bx = i < g.n_box;
    ux0 = std::min(ux0, p[0]), ux1 = std::max(ux1, bx ? p[3] : p[1]);
    uz0 = std::min(uz0, p[2]), uz1 = std::max(uz1, bx ? p[5] : p[3]);
  }
  d.ox0 = ux0 - mo, d.ox1 = ux1 + mo, d.oz0 = uz0 - mo, d.oz1 = uz1 + mo;
  out.assign(sizeof(DPlanes) / 4, 0u);
  std::memcpy(out.data(), &d, sizeof d);
  return true;
}

// Where the blocks keep what (ScenePlacement), from the compiled trees and tables.
int plan_placement(const rt_scene_desc* d, int32_t placement, const SceneTuning& tune, const BuiltTree& tree,
                   const std::vector<DNode4F>& nodes4, int32_t stack4, float origin_limit, CompiledScene& cs,
                   std::string* err) {
  ScenePlacement& P = cs.place;
  const bool ext = !cs.exts.empty();
  const int n_nodes4 = (int)nodes4.size(), n_mats = (int)cs.mats.size(), n_texs = (int)cs.texs.size();
  P.stack_depth4 = stack4;
  P.root4 = (nodes4[0].child[0] >= 0 && nodes4[0].child[0] != kEmptyChild) ? nodes4[0].child[0] : 0;
  {
    int kbits = 1;
    while ((size_t)1 << kbits < nodes4.size()) ++kbits;
    if (kbits > kMaxKeyBits) return fail(err, RT_E_UNSUPPORTED, "BVH too large (%zu 4-wide nodes)", nodes4.size());
    P.key_mask = (1u << kbits) - 1u;
  }
  P.origin_limit = origin_limit;
  const int32_t depth = tree_branch_depth(tree);
  P.stack_depth = depth + 2;  // ordered traversal holds at most one deferred child per branch level
  // LDS of one block: the traversal stacks, then a copy of (the top levels of) the BVH.
  // Megakernel (4-wide tree): the whole tree in LDS with one kTraceThreadsWide block per CU when it
  // fits beside the stacks (MI355X: 160 KiB per CU), else kTraceThreads blocks reading nodes
  // through L1/L2.  rt_scene_hit (2-wide tree): placement flags only.
  auto lds_count = [&](long long stack, size_t node_bytes, size_t n) -> int32_t {
    long long room = std::min<long long>((kLdsBytes - stack) / (long long)node_bytes, (long long)n);
    if (placement & RT_BVH_NODES_LDS) return (int32_t)room;
    if (placement & RT_BVH_NODES_HALF_LDS) return (int32_t)std::min<long long>(room, (long long)n / 2);
    if (tune.has_lds_nodes) return (int32_t)std::min<long long>(room, tune.lds_nodes);  // tuning
    return 0;  // nodes read through L1/L2
  };
  auto lds_nodes_for = [&](long long stack) { return lds_count(stack, sizeof(DNode), cs.nodes.size()); };
  P.stack_bytes = (long long)P.stack_depth * kTraceThreads * 8;
  const long long stack4_bytes = (long long)trace_lds_bytes(0, 0, 0, 0, stack4, kTraceThreads, 0, 0);
  // book-2 scenes: the EXT instance spills ~80 VGPRs at 4 waves per SIMD (1024 threads) and none at 3
  // (768 threads, 165 VGPRs): final_scene +3.3 % (profiles/r02/wide3.txt), so no 1024-thread EXT instance
  // is built.  The wide block's LDS holds the tree plus one stack per thread of the block actually launched.
  const int wide_threads = ext ? kTraceThreadsWide3 : kTraceThreadsWide;
  const int n4_bytes = node4_bytes(ext);
  // the wide block's LDS with the tree alone / with the primitives and the material and texture tables /
  // with the Perlin tables too
  auto wide_lds = [&](int n_prims, int n_perlin, int mats, int texs) {
    return trace_lds_bytes(n_nodes4, n4_bytes, n_prims, n_perlin, stack4, wide_threads, mats, texs);
  };
  if (P.stack_bytes > kLdsBytes || stack4_bytes > kLdsBytes)
    return fail(err, RT_E_UNSUPPORTED, "BVH too deep for the LDS traversal stack (depth %d)", depth);
  P.wide = wide_lds(0, 0, 0, 0) <= (size_t)kLdsBytes && (placement == 0 || placement == RT_BVH_NODES_LDS) &&
           !tune.no_wide;  // tuning
  P.mk_threads = P.wide ? wide_threads : kTraceThreads;
  P.n_lds_nodes = lds_nodes_for(kHitThreads * 8LL * P.stack_depth);
  P.n_lds_nodes4 = P.wide ? n_nodes4 : lds_count(stack4_bytes, n4_bytes, nodes4.size());
  // primitives too, with the material and texture tables (the megakernel's scene-in-LDS instance reads all
  // three from LDS), when they fit beside the wide block's tree and stacks
  const bool prims_lds = P.wide && wide_lds(d->n_objects, 0, n_mats, n_texs) <= (size_t)kLdsBytes &&
                         !tune.no_lds_prims && !tune.no_lds_mats;
  P.n_lds_prims = prims_lds ? d->n_objects : 0;
  // and the Perlin tables (marble's ~210 gathers per evaluation from LDS)
  const bool perlin_lds = prims_lds && d->n_perlin > 0 &&
                          wide_lds(d->n_objects, d->n_perlin, n_mats, n_texs) <= (size_t)kLdsBytes &&
                          !tune.no_lds_perlin;
  P.n_lds_perlin = perlin_lds ? d->n_perlin : 0;
  // the material and texture tables ride with the primitives (the record / shading reads: headline +1.0 %,
  // Cornell +0.7 %; SHIRLEY_NO_LDS_MATS keeps all three in global memory).  The wavefront and
  // split engines keep their own LDS layouts and read them from global memory (their scene copies carry
  // n_lds_mats = 0).
  P.n_lds_mats = prims_lds ? n_mats : 0;
  P.n_lds_texs = prims_lds ? n_texs : 0;
  // the hop pass (trace.hip): a reference scene in the scene-in-LDS instance that holds a RectBox with a
  // dielectric material — the thin coat whose one-visit segments the pass serves (SHIRLEY_NO_HOP: never)
  bool coat = false;
  for (int i = 0; i < d->n_objects && !coat; ++i) {
    const rt_object& o = d->objects[i];
    coat = o.geometry == RT_GEOM_RECT_BOX && d->materials[o.material].kind == RT_MAT_DIELECTRIC;
  }
  P.hop_pass = coat && !ext && prims_lds && !tune.no_hop;  // tuning
  // ... by the scene's ground stack where it has one (SHIRLEY_HOP=root: never), else by a first-node visit
  GroundConsts consts;
  P.hop_kind = !P.hop_pass ? 0 : (!tune.hop_root && ground_stack(cs.prims, d->n_objects, cs.ground, &consts)) ? 2 : 1;
  if (P.hop_kind != 2) cs.ground.clear();
  // ... and, before the sampler, the downward hops too (trace.hip, HOP = 3) where the stack holds a primitive the
  // down pass can find: one of another material on a plane at least `gap` below Y (SHIRLEY_HOP=up: never)
  P.hop_down = false;
  if (P.hop_kind == 2 && !tune.hop_up) {
    DGround g;
    std::memcpy(&g, cs.ground.data(), sizeof g);
    for (int i = 0; i < g.n && !P.hop_down; ++i) {
      const DPrim& q = cs.prims[g.prim[i]];
      if (cs.mats[q.material].kind == RT_MAT_DIELECTRIC) continue;
      // (a rect by the top of its padded box, as ground_hop_t does: a raised rect that makes the top plane is on Y)
      P.hop_down = i < g.n_box ? (q.p[1] <= g.y_down || q.p[4] <= g.y_down) : q.p[4] + 0.0001 <= g.y_down;
    }
  }
  // ... both by the closed-form next plane (trace.hip, HOP = 4) where the stack is a plane stack (SHIRLEY_HOP=general:
  // never); a stack that misses a premise keeps the general passes
  P.hop_planes = P.hop_down && !tune.hop_general && plane_stack(cs.prims, cs.mats, cs.ground, consts, cs.planes);
  if (P.hop_planes) {
    // plane_first's premise (the HOP = 4 instances skip every rect and RectBox leaf of a lane it answered): each of
    // them belongs to G — ground_stack admits no other, so this only fails if that rule changes
    DGround g;
    std::memcpy(&g, cs.ground.data(), sizeof g);
    int n_flat = 0;
    for (int i = 0; i < d->n_objects; ++i) n_flat += cs.prims[i].kind != kPrimSphere;
    assert(n_flat == g.n);
    if (n_flat != g.n) P.hop_planes = false;
  }
  if (!P.hop_planes) cs.planes.clear();

  // wavefront extend block: its own (larger) stack area, the rest of LDS for nodes
  const long long wf_stack = (long long)wf_extend_lds(0, P.stack_depth);
  if (wf_stack > kLdsBytes)
    return fail(err, RT_E_UNSUPPORTED, "BVH too deep for the LDS traversal stack (depth %d)", depth);
  P.wf_n_lds_nodes = lds_nodes_for(wf_stack);
  P.wf_extend4 = P.wide && P.n_lds_prims > 0 && !tune.wf_extend2;
  // RT_ENGINE_SPLIT: the wide block's scene plus traversal stacks and ray slots in LDS
  if (P.wide && !ext && P.n_lds_prims == d->n_objects) {
    P.split_nt = tune.split_nt;            // tuning
    P.split_refill = tune.split_refill;    // tuning
  }

  cs.stats.n_objects = d->n_objects;
  cs.stats.n_nodes = (int32_t)tree.nodes.size();
  int32_t leaves = 0;
  for (const auto& n : tree.nodes) leaves += n.leaf >= 0;
  cs.stats.n_leaves = leaves;
  cs.stats.depth = depth;
  cs.stats.n_nodes4 = n_nodes4;
  cs.stats.wide_block = P.wide ? 1 : 0;
  cs.stats.origin_limit = P.origin_limit;
  cs.stats.hop_pass = P.hop_pass ? 1 : 0;
  cs.stats.hop_kind = P.hop_kind;
  cs.stats.device_bytes = (int64_t)(cs.nodes.size() * sizeof(DNode) + cs.prims.size() * sizeof(DPrim) +
                                    cs.mats.size() * sizeof(DMat) + cs.texs.size() * sizeof(DTex) +
                                    cs.perlin.size() * sizeof(DPerlin) + cs.texels.size());
  return RT_OK;
}

}  // namespace

// The listing rule of include/shirley_rt.h (rt_scene_lights), object by object.
LightList list_lights(const rt_scene_desc* d) {
  LightList out;
  for (int i = 0; i < d->n_objects; ++i) {
    const rt_object& o = d->objects[i];
    const rt_material& m = d->materials[o.material];
    if (m.kind != RT_MAT_DIFFUSE_LIGHT && m.kind != RT_MAT_FAIRY_LIGHT) continue;
    const rt_texture& t = d->textures[m.texture];
    const bool rect = o.geometry == RT_GEOM_RECT_XY || o.geometry == RT_GEOM_RECT_YZ || o.geometry == RT_GEOM_RECT_XZ;
    bool listed = t.kind == RT_TEX_SOLID && !o.medium && !o.transform;
    double area = 0.0;
    if (rect) {
      const double e1 = o.p[1] - o.p[0], e2 = o.p[3] - o.p[2];
      listed = listed && e1 > 0.0 && e2 > 0.0;
      area = e1 * e2;
    } else if (o.geometry == RT_GEOM_SPHERE) {
      listed = listed && o.p[3] > 0.0;
      area = (4.0 * 3.141592653589793) * (o.p[3] * o.p[3]);
    } else {
      listed = false;
    }
    if (!listed) {
      ++out.n_unlisted;
      continue;
    }
    rt_light l{};
    l.object = i;
    l.geometry = o.geometry;
    l.emitter = m.kind;
    l.area = area;
    DLight dl{};
    dl.geometry = o.geometry;
    dl.emitter = m.kind;
    for (int k = 0; k < 6; ++k) dl.p[k] = o.p[k];
    dl.area = area;
    for (int k = 0; k < 3; ++k) l.color[k] = dl.color[k] = t.color[k];
    out.lights.push_back(l);
    out.dev.push_back(dl);
  }
  return out;
}

// The light grid of include/shirley_rt.h (rt_scene_light_pick), step by step in the header's order: + - * /,
// comparisons and selects only (no libm; the build never fuses a * b + c).
// With `masks` (rt_scene_light_visibility: [cells][L] words of `rays` bits each), a cell that has a live point
// builds its row from w'_j = w_j * v_j, v_j the smoothed share of the cell's live points that see light j.
int build_light_grid(const LightList& l, int32_t cells, bool want_cdf, LightGridTable* out, const uint32_t* masks,
                     int32_t rays) {
  *out = LightGridTable{};
  if (cells < 1 || cells > kLightGridMaxCells) return RT_E_INVALID;
  const size_t L = l.dev.size();
  if (L == 0) return RT_OK;
  // per light: its box, its centre, rho2 and Phi
  struct Item {
    double lo[3], hi[3], c[3], rho2, phi;
  };
  std::vector<Item> items(L);
  rt_light_grid& g = out->info;
  for (size_t j = 0; j < L; ++j) {
    const DLight& q = l.dev[j];
    Item& it = items[j];
    if (q.geometry == RT_GEOM_SPHERE) {
      const double r = q.p[3];
      for (int a = 0; a < 3; ++a) {
        it.c[a] = q.p[a];
        it.lo[a] = q.p[a] - r;
        it.hi[a] = q.p[a] + r;
      }
      it.rho2 = r * r;
    } else {
      // (d1, d2, axis): RECT_XY (x, y, z), RECT_YZ (y, z, x), RECT_XZ (x, z, y)
      const int d1 = q.geometry == RT_GEOM_RECT_YZ ? 1 : 0;
      const int d2 = q.geometry == RT_GEOM_RECT_XY ? 1 : 2;
      const int ax = 3 - d1 - d2;
      const double h1 = (q.p[1] - q.p[0]) * 0.5, h2 = (q.p[3] - q.p[2]) * 0.5;
      it.lo[d1] = q.p[0];
      it.hi[d1] = q.p[1];
      it.c[d1] = q.p[0] + h1;
      it.lo[d2] = q.p[2];
      it.hi[d2] = q.p[3];
      it.c[d2] = q.p[2] + h2;
      it.lo[ax] = it.hi[ax] = it.c[ax] = q.p[4];
      it.rho2 = h1 * h1 + h2 * h2;
    }
    const double s = (q.color[0] + q.color[1]) + q.color[2];
    it.phi = q.area * (s > 0.0 ? s : 0.0);  // (a NaN sum gives 0)
    for (int a = 0; a < 3; ++a) {
      g.lo[a] = (j == 0 || it.lo[a] < g.lo[a]) ? it.lo[a] : g.lo[a];
      g.hi[a] = (j == 0 || it.hi[a] > g.hi[a]) ? it.hi[a] : g.hi[a];
    }
  }
  // dimensions: `cells` along the longest axis, in proportion on the others, 1 on a flat one
  double ext[3], ext_max = 0.0;
  for (int a = 0; a < 3; ++a) {
    ext[a] = g.hi[a] - g.lo[a];
    ext_max = (a == 0 || ext[a] > ext_max) ? ext[a] : ext_max;
  }
  int64_t n_cells = 1;
  double size[3];
  for (int a = 0; a < 3; ++a) {
    if (!(ext[a] > 0.0)) {
      g.n[a] = 1;
    } else {
      const double f = (double)cells * (ext[a] / ext_max);
      g.n[a] = f < (double)cells ? 1 + (int32_t)f : cells;  // = min(cells, 1 + (int)f); a NaN gives cells
    }
    size[a] = ext[a] / (double)g.n[a];
    n_cells *= g.n[a];
  }
  g.n_lights = (int32_t)L;
  if (n_cells * (int64_t)L > kLightGridMaxEntries) {
    *out = LightGridTable{};
    return RT_E_INVALID;
  }
  if (!want_cdf) return RT_OK;
  out->cdf.resize((size_t)n_cells * L);
  const double diag2 = (size[0] * size[0] + size[1] * size[1]) + size[2] * size[2];
  const double floor_p = kLightPickUniform / (double)L;
  std::vector<double> w(L);
  double* row = out->cdf.data();
  for (int32_t iz = 0; iz < g.n[2]; ++iz)
    for (int32_t iy = 0; iy < g.n[1]; ++iy)
      for (int32_t ix = 0; ix < g.n[0]; ++ix, row += L) {
        const int32_t idx[3] = {ix, iy, iz};
        double clo[3], chi[3];
        for (int a = 0; a < 3; ++a) {
          clo[a] = g.lo[a] + (double)idx[a] * size[a];
          chi[a] = g.lo[a] + (double)(idx[a] + 1) * size[a];
        }
        double W = 0.0;
        for (size_t j = 0; j < L; ++j) {
          const Item& it = items[j];
          double dd[3];
          for (int a = 0; a < 3; ++a) {
            double t = clo[a] - it.c[a];
            t = t > 0.0 ? t : 0.0;
            const double e = it.c[a] - chi[a];
            dd[a] = e > t ? e : t;
          }
          const double D2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2];
          const double m = it.rho2 + diag2;
          w[j] = it.phi / (D2 > m ? D2 : m);
          W = W + w[j];
        }
        if (masks) {
          const uint32_t field = rays >= 32 ? 0xFFFFFFFFu : (1u << rays) - 1u;
          const uint32_t* m = masks + (size_t)(row - out->cdf.data());
          uint32_t valid = 0;
          for (size_t j = 0; j < L; ++j) valid |= m[j] & field;
          const int Kc = __builtin_popcount(valid);  // the cell's live points: those some light sees
          if (Kc) {
            W = 0.0;
            for (size_t j = 0; j < L; ++j) {
              const double v = ((double)__builtin_popcount(m[j] & field) + 1.0) / ((double)Kc + 2.0);
              w[j] = w[j] * v;
              W = W + w[j];
            }
          }
        }
        // (W is 0, +inf or a NaN: the uniform row)
        const bool weighted = W > 0.0 && W < std::numeric_limits<double>::infinity();
        double acc = 0.0;
        for (size_t j = 0; j < L; ++j) {
          if (weighted) {
            acc = acc + (((w[j] / W) * kLightPickWeighted) + floor_p);
            row[j] = acc;
          } else {
            row[j] = (double)(j + 1) / (double)L;
          }
        }
        row[L - 1] = 1.0;
      }
  return RT_OK;
}

// The path's draw `draw` of (seed, pixel, sample): Philox4x32-10 at counter (draw / 2, sample, pixel, 0), the low
// word pair for an even draw and the high pair for an odd one, converted as (u64 >> 11) * 2^-53 (rt_device.h).
double path_draw(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t draw) {
  uint32_t c[4] = {draw >> 1, sample, pixel, 0u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
  }
  const uint64_t v = (draw & 1u) ? ((uint64_t)c[2] | ((uint64_t)c[3] << 32)) : ((uint64_t)c[0] | ((uint64_t)c[1] << 32));
  return (double)(v >> 11) * (1.0 / 9007199254740992.0);
}

// One ray of rt_scene_light_visibility in the header's order (lightvis.hip is the device's form).
bool light_visibility_ray(const rt_light_grid& g, const DLight& q, uint64_t seed, uint32_t cell, uint32_t light,
                          uint32_t i, double* x, double* w) {
  const uint32_t nx = (uint32_t)g.n[0], ny = (uint32_t)g.n[1];
  const uint32_t iz = cell / (nx * ny), iy = (cell - iz * (nx * ny)) / nx, ix = cell - (iz * ny + iy) * nx;
  const uint32_t idx[3] = {ix, iy, iz};
  for (int a = 0; a < 3; ++a) {
    const double size = (g.hi[a] - g.lo[a]) / (double)g.n[a];
    x[a] = (g.lo[a] + (double)idx[a] * size) + path_draw(seed, cell, i, (uint32_t)a) * size;
  }
  double y[3];
  if (q.geometry == RT_GEOM_SPHERE) {
    const double r = q.p[3];
    const double e[3] = {x[0] - q.p[0], x[1] - q.p[1], x[2] - q.p[2]};
    const double e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    if (!(e2 > r * r)) {
      w[0] = w[1] = w[2] = 0.0;
      return false;
    }
    const double le = std::sqrt(e2);
    for (int a = 0; a < 3; ++a) y[a] = q.p[a] + r * (e[a] / le);
  } else {
    const int d1 = q.geometry == RT_GEOM_RECT_YZ ? 1 : 0;
    const int d2 = q.geometry == RT_GEOM_RECT_XY ? 1 : 2;
    const double xi1 = path_draw(seed, cell, i, 4u + 2u * light);
    const double xi2 = path_draw(seed, cell, i, 5u + 2u * light);
    y[d1] = q.p[0] + xi1 * (q.p[1] - q.p[0]);
    y[d2] = q.p[2] + xi2 * (q.p[3] - q.p[2]);
    y[3 - d1 - d2] = q.p[4];
  }
  for (int a = 0; a < 3; ++a) w[a] = y[a] - x[a];
  return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2] > 0.0;
}

int compile_scene(const rt_scene_desc* d, int32_t builder, const SceneTuning& tune, CompiledScene* out,
                  std::string* err) {
  int st = validate(d, err);
  if (st) return st;
  const int32_t placement = builder & kPlacementMask;
  builder &= ~kPlacementMask;
  if (builder != RT_BVH_REFERENCE && builder != RT_BVH_SAH) return fail(err, RT_E_INVALID, "bad bvh builder %d", builder);
  if (d->n_objects > kLeafPrimMask) return fail(err, RT_E_UNSUPPORTED, "too many objects (%d)", d->n_objects);
  *out = CompiledScene{};
  CompiledScene& cs = *out;
  cs.digest = scene_digest(d, builder);  // (of the description as given)
  cs.lights = list_lights(d);            // (likewise: rt_light.object indexes the caller's objects)
  std::vector<rt_object> flat;
  const rt_scene_desc fd = flat_scene(d, flat);
  for (int i = 0; i < d->n_objects; ++i)
    if (d->objects[i].rotate_y_deg != 0.0 && flattens(d, d->objects[i])) {
      double cos_t, sin_t;
      rotate_y_cs(d->objects[i], cos_t, sin_t);
      cs.uv_fixups.push_back({i, {cos_t, sin_t}});
    }
  d = &fd;

  BuiltTree tree = build_tree(d, builder, tune);
  // Exact ties (rt_device.h tie_takes): the device numbers the primitives in the reference
  // tree's leaf order, lhs before rhs (constructor.rs:9-36 via build_reference_tree), so that the lower
  // number is the leaf the reference's rhs-first walk tests last; prim_object maps a number back.
  std::vector<rt_object> ranked;
  rt_scene_desc rd = *d;
  {
    const BuiltTree ref = builder == RT_BVH_REFERENCE ? tree : build_tree(d, RT_BVH_REFERENCE, tune);
    std::vector<int32_t> rank = reference_ranks(ref, d->n_objects);
    ranked.resize((size_t)std::max(0, d->n_objects));
    cs.prim_object.assign((size_t)std::max(0, d->n_objects), 0);
    for (int i = 0; i < d->n_objects; ++i) {
      ranked[rank[i]] = d->objects[i];
      cs.prim_object[rank[i]] = i;
    }
    for (BuildNode& nd : tree.nodes)
      if (nd.leaf >= 0) nd.leaf = rank[nd.leaf];
    rd.objects = ranked.data();
    d = &rd;
    // (a listed light is no instance, so flat_scene left it at its index)
    cs.prim_light.assign(std::max<size_t>(1, cs.prim_object.size()), -1);
    for (size_t j = 0; j < cs.lights.lights.size(); ++j) cs.prim_light[rank[cs.lights.lights[j].object]] = (int32_t)j;
  }
  flatten(tree, cs.nodes);
  std::vector<DNode4F> nodes4;
  int32_t stack4 = 1;
  const Inflation infl = inflation_for(tree);
  flatten4(tree, d, infl.delta, nodes4, stack4, false);
  std::vector<DPrim>& prims = cs.prims;
  std::vector<DExt>& exts = cs.exts;
  prims.resize(std::max(1, d->n_objects));
  for (int i = 0; i < d->n_objects; ++i) {
    const rt_object& o = d->objects[i];
    DPrim& q = prims[i];
    std::memset(&q, 0, sizeof q);
    for (int k = 0; k < 6; ++k) q.p[k] = o.p[k];
    q.kind = o.geometry == RT_GEOM_SPHERE     ? kPrimSphere
             : o.geometry == RT_GEOM_RECT_XY  ? kPrimRectXY
             : o.geometry == RT_GEOM_RECT_YZ  ? kPrimRectYZ
             : o.geometry == RT_GEOM_RECT_XZ  ? kPrimRectXZ
             : o.geometry == RT_GEOM_RECT_BOX ? kPrimBox
                                              : kPrimMovingSphere;
    // a sphere's 1 / radius (sphere.rs:48 `scale(1.0 / self.radius)`), the same IEEE quotient the device
    // would compute per hit record; p[4] is otherwise unused by spheres
    if (q.kind == kPrimSphere || q.kind == kPrimMovingSphere) q.p[4] = 1.0 / q.p[3];
    if (q.kind == kPrimSphere) {
      // the sure-pass bound of the sphere's box test (rt_device.h leaf_tests4): r - eta rounded down, eta =
      // 2^-48 (B + L) (B the largest box plane, L the fast-ray origin bound), or 0 (never sure)
      const double eta = std::ldexp(infl.box_bound + (double)infl.origin_limit, -48);
      const double rs = q.p[3] - eta;
      q.p[5] = (std::isfinite(rs) && rs > 0.0) ? std::nextafter(rs, 0.0) : 0.0;
    }
    q.material = o.material;
    if (is_extended(o)) {
      if (exts.size() >= (1u << (31 - kPrimExtShift)))
        return fail(err, RT_E_UNSUPPORTED, "too many extended objects");
      DExt e{};
      box_to6(object_box(o), e.box);
      for (int k = 0; k < 3; ++k) e.c1[k] = o.q[k];
      e.t0 = o.q[3];
      e.t1 = o.q[4];
      e.cos_t = 1.0;
      if (o.transform) {
        rotate_y_cs(o, e.cos_t, e.sin_t);
        for (int k = 0; k < 3; ++k) e.off[k] = o.offset[k];
      }
      e.neg_inv_density = -1.0 / o.density;
      e.object = cs.prim_object[i];
      e.prim = i;
      q.kind |= kPrimExt | (o.medium ? kPrimMedium : 0) | (o.transform ? kPrimXform : 0) |
                ((int32_t)exts.size() << kPrimExtShift);
      exts.push_back(e);
    }
  }
  std::vector<DMat>& mats = cs.mats;
  mats.resize(std::max(1, d->n_materials));
  for (int i = 0; i < d->n_materials; ++i) {
    const rt_material& m = d->materials[i];
    DMat& q = mats[i];
    std::memset(&q, 0, sizeof q);
    q.kind = m.kind;
    q.tex = m.texture;
    for (int k = 0; k < 3; ++k) q.albedo[k] = m.albedo[k];
    q.param = m.param;
    q.inv_param = 1.0 / m.param;  // IEEE division: the bits dielectric.rs:27 computes per hit
    if (m.kind == RT_MAT_DIELECTRIC) {
      // Schlick's r0^2 (dielectric.rs:15-19) for the two ratios a hit can have — front face 1 / ir, back face
      // ir — with the reference's operations (host and device are both IEEE binary64 without contraction), so
      // the megakernel's reflectance skips a division per hit; a dielectric has no albedo (its attenuation is 1)
      const double ratios[2] = {q.inv_param, m.param};
      for (int k = 0; k < 2; ++k) {
        double r0 = (1.0 - ratios[k]) / (1.0 + ratios[k]);
        q.albedo[k] = r0 * r0;
      }
      q.albedo[2] = 0.0;
    }
  }
  // every image's RGB8 texels in one pool; an image texture's DTex points at its image (rt_scene_upload, once
  // the pool is on the device)
  std::vector<size_t>& img_off = cs.img_off;
  std::vector<uint8_t>& texels = cs.texels;
  img_off.resize(std::max(1, d->n_images));
  for (int i = 0; i < d->n_images; ++i) {
    img_off[i] = texels.size();
    size_t nb = (size_t)d->images[i].width * d->images[i].height * 3;
    texels.insert(texels.end(), d->images[i].rgb, d->images[i].rgb + nb);
  }
  if (texels.empty()) texels.resize(16);
  std::vector<DTex>& texs = cs.texs;
  texs.resize(std::max(1, d->n_textures));
  for (int i = 0; i < d->n_textures; ++i) {
    const rt_texture& t = d->textures[i];
    DTex& q = texs[i];
    std::memset(&q, 0, sizeof q);
    q.kind = t.kind;
    q.odd = t.odd;
    q.even = t.even;
    q.table = t.table;
    if (t.kind != RT_TEX_IMAGE)
      for (int k = 0; k < 3; ++k) q.color[k] = t.color[k];
    q.scale = t.scale;
    if (t.kind == RT_TEX_IMAGE) {  // (validated: a texture's image index is in range)
      q.img.width = d->images[t.table].width;
      q.img.height = d->images[t.table].height;
    }
    cs.has_perlin |= t.kind == RT_TEX_PERLIN;
  }
  std::vector<DPerlin>& perl = cs.perlin;
  perl.resize(std::max(1, d->n_perlin));
  for (int i = 0; i < d->n_perlin; ++i) {
    std::memcpy(perl[i].ranfloat, d->perlin[i].ranfloat, sizeof perl[i].ranfloat);
    std::memcpy(perl[i].perm_x, d->perlin[i].perm_x, sizeof perl[i].perm_x);
    std::memcpy(perl[i].perm_y, d->perlin[i].perm_y, sizeof perl[i].perm_y);
    std::memcpy(perl[i].perm_z, d->perlin[i].perm_z, sizeof perl[i].perm_z);
  }
  cs.n_perlin = d->n_perlin;

  // The 4-wide collapse: the optimal one (fewest expected node visits by area) for a reference scene that
  // will run in the scene-in-LDS instance — Cornell +15 %, headline +0.3 % — and the greedy one for the
  // scenes read through L1/L2 (gen_spheres −1.4 %, final_scene −1.6 % with the optimal one).
  // The same test as the placement (plan_placement: tree, stacks, primitives and tables within the wide
  // block's LDS), on either tree, but always for DNode4F nodes and a kTraceThreadsWide block.
  // SHIRLEY_COLLAPSE_DP=1 / =0: always / never (tuning).
  {
    auto scene_in_lds = [&](const std::vector<DNode4F>& n4, int32_t s4) {
      return trace_lds_bytes((int)n4.size(), (int)sizeof(DNode4F), d->n_objects, 0, s4, kTraceThreadsWide,
                             (int)mats.size(), (int)texs.size()) <= (size_t)kLdsBytes;
    };
    const bool forced = tune.collapse_dp >= 0;
    const bool want = forced ? tune.collapse_dp != 0
                             : (exts.empty() && (placement == 0 || placement == RT_BVH_NODES_LDS) && scene_in_lds(nodes4, stack4));
    if (want) {
      std::vector<DNode4F> dp4;
      int32_t dp_stack = 1;
      flatten4(tree, d, infl.delta, dp4, dp_stack, true);
      if (forced || scene_in_lds(dp4, dp_stack)) {
        nodes4.swap(dp4);
        stack4 = dp_stack;
        cs.place.collapse_dp = true;
      }
    }
  }
  // book-2 scenes run the EXT kernel instances, which read the compact node layout (rt_layout.h)
  if (exts.empty()) {
    cs.nodes4.resize(nodes4.size() * sizeof(DNode4F));
    std::memcpy(cs.nodes4.data(), nodes4.data(), cs.nodes4.size());
  } else {
    std::vector<DNode4C> compact(nodes4.size());
    for (size_t i = 0; i < nodes4.size(); ++i) {
      for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 4; ++k) {
          compact[i].lo[a][k] = nodes4[i].row[a][0][k];
          compact[i].hi[a][k] = nodes4[i].row[a][1][k];
        }
      for (int k = 0; k < 4; ++k) compact[i].child[k] = nodes4[i].child[k];
    }
    cs.nodes4.resize(compact.size() * sizeof(DNode4C));
    std::memcpy(cs.nodes4.data(), compact.data(), cs.nodes4.size());
  }
  return plan_placement(d, placement, tune, tree, nodes4, stack4, infl.origin_limit, cs, err);
}

}  // namespace rt
