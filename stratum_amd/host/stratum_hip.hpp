// stratum_hip.hpp — C++ host side above the C ABI (include/sthip.h): the slice of Stratum's host
// interface that feeds and drives the path-tracing hot path, with the reference's own names, argument
// meaning and error behaviour (exceptions), so that host code written against Stratum keeps compiling:
//
//   stm::NodeGraph / Node / component_ptr<T> / Node::Event     src/Node/NodeGraph.hpp:13-360
//   stm::TransformData helpers, make_perspective, quatf        src/Shaders/transform.h, quatf.h
//   stm::Material, Mesh, MeshPrimitive, Camera                 src/Node/Material.hpp, Scene.hpp:15-37
//   stm::node_to_world                                         src/Node/Scene.cpp:108-117
//   stm::Application (OnUpdate / OnRenderWindow only)          src/Node/Application.hpp:11-29
//   stm::Scene  (update() packs SceneData, data())             src/Node/Scene.hpp:44-69, Scene.cpp:299-684
//   stm::Denoiser (denoise(), reset_accumulation())            src/Node/Denoiser.hpp:9-60, Denoiser.cpp:117-274
//   stm::BDPT   (update(), render(), prev_result())            src/Node/BDPT.hpp:13-24, BDPT.cpp:35-127,341-838
//
// What is NOT here: Vulkan (Device, CommandBuffer, Image, Buffer), loaders, GUI, window. The
// CommandBuffer& parameters of the reference's signatures become an opaque stm::CommandBuffer that carries
// the HIP stream. The reference needs Eigen for its vector types; this header uses plain arrays (Eigen is
// not in the image), so float3 etc. are minimal structs.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <queue>
#include <stdexcept>
#include <string>
#include <tuple>
#include <typeindex>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include <dlfcn.h>

#include "../../include/sthip.h"
// A library that cannot refit lacks this symbol (include/sthip.h): a weak reference, so that the host links against it
// all the same and BDPT::update probes for the call before using it.
#pragma weak sthip_scene_update_vertices
// ... and one that cannot pose rigs on the device lacks these: Scene::update then poses them on the host
#pragma weak sthip_scene_set_rigs
#pragma weak sthip_scene_animate
#pragma weak sthip_scene_read_vertices
// ... and one without 8-bit resident textures lacks these: Scene::update then converts such images to float on the host
#pragma weak sthip_scene_upload_formats
#pragma weak sthip_scene_read_image
// ... and one without the post block lacks these: Denoiser::denoise then throws
// ... and one without the material conversions lacks this: Scene::make_*_material then throw for a material with images
#pragma weak sthip_convert_material
#pragma weak sthip_decode_texels
// ... and one that cannot replace the environment of a resident scene lacks these: the host builds the tables and uploads
#pragma weak sthip_scene_set_environment
#pragma weak sthip_scene_read_distributions
// ... and one that cannot edit the materials of a resident scene lacks these: a changed colour or texture is an upload
#pragma weak sthip_scene_set_images
#pragma weak sthip_scene_set_material_data
#pragma weak sthip_scene_read_image_range
// ... and one that cannot take instance matrices from device memory or build the top level there lacks these
// ... and one that cannot build a density grid on the device or replace a resident one lacks these: a Medium's dense source
// then needs a finished grid from the host, and a changed grid is an upload
#pragma weak sthip_build_volume
#pragma weak sthip_scene_set_volume
#pragma weak sthip_scene_read_volume
#pragma weak sthip_scene_set_transforms
#pragma weak sthip_scene_read_transforms
#pragma weak sthip_scene_read_top_level
// ... and one that cannot take vertices from device streams lacks this: BDPT::set_vertices_device then throws
#pragma weak sthip_scene_set_vertices
#pragma weak sthip_accumulate
#pragma weak sthip_denoise_filter
#include "../../include/sthip_detmath.h"  // det_f16tof32: export_hdr of a half frame

namespace stm {

// ------------------------------------------------------------------------------------------------
// NodeGraph.hpp:13-360
// ------------------------------------------------------------------------------------------------
class Node;
class NodeGraph;

template <typename T>
class component_ptr {
 public:
  component_ptr() = default;
  component_ptr(std::nullptr_t) {}
  component_ptr(Node* n, T* c) : mNode(n), mComponent(c) {}
  component_ptr(const Node* n, T* c) : mNode(const_cast<Node*>(n)), mComponent(c) {}
  Node& node() const { return *mNode; }
  operator bool() const { return mComponent != nullptr; }
  T& operator*() const { return *mComponent; }
  T* operator->() const { return mComponent; }
  T* get() const { return mComponent; }
  void reset() {
    mNode = nullptr;
    mComponent = nullptr;
  }

 private:
  Node* mNode = nullptr;
  T* mComponent = nullptr;
};

class NodeGraph {
 public:
  bool empty() const { return mNodes.empty(); }
  bool contains(const Node* ptr) const { return mNodes.count(ptr) != 0; }
  inline Node& emplace(const std::string& name);
  inline void erase(Node& node);
  template <typename T>
  size_t component_count() const {
    auto it = mComponentMap.find(typeid(T));
    return it == mComponentMap.end() ? 0 : it->second.mComponents.size();
  }
  inline ~NodeGraph();

 private:
  friend class Node;
  struct component_map {
    void (*mDestructor)(const void*);
    std::unordered_map<const Node*, void*> mComponents;
  };
  std::unordered_map<const Node*, std::unique_ptr<Node>> mNodes;
  std::unordered_map<std::type_index, component_map> mComponentMap;
};

class Node {
 public:
  enum EventPriority : uint32_t { eFirst = 0, eAlmostFirst = 0x3FFFFFFF, eDefault = 0x7FFFFFFF, eAlmostLast = 0xBFFFFFFD, eLast = 0xFFFFFFFF };

  template <typename... Args>
  class Event {
   public:
    using function_t = std::function<void(Args...)>;
    void clear() { mListeners.clear(); }
    bool empty() const { return mListeners.empty(); }
    void add_listener(const Node& node, function_t&& fn, uint32_t priority = EventPriority::eDefault) {
      mListeners.emplace_back(&node, std::move(fn), priority);
      std::stable_sort(mListeners.begin(), mListeners.end(), [](const auto& a, const auto& b) { return std::get<2>(a) < std::get<2>(b); });
      if (!mNodeGraph) mNodeGraph = &node.node_graph();
    }
    void erase(const Node& node) {
      for (auto it = mListeners.begin(); it != mListeners.end();) it = (std::get<0>(*it) == &node) ? mListeners.erase(it) : it + 1;
    }
    void operator()(Args... args) const {
      auto tmp = mListeners;  // listeners may add/remove listeners
      for (const auto& l : tmp)
        if (mNodeGraph->contains(std::get<0>(l))) std::get<1>(l)(args...);
    }

   private:
    const NodeGraph* mNodeGraph = nullptr;
    std::vector<std::tuple<const Node*, function_t, uint32_t>> mListeners;
  };

  Node(const Node&) = delete;
  ~Node() {
    for (const std::type_index& t : mComponents) {
      auto& cm = mNodeGraph.mComponentMap.at(t);
      auto it = cm.mComponents.find(this);
      if (it != cm.mComponents.end()) {
        cm.mDestructor(it->second);
        cm.mComponents.erase(it);
      }
    }
  }

  const std::string& name() const { return mName; }
  NodeGraph& node_graph() const { return mNodeGraph; }
  Node* parent() const { return mParent; }
  // children in insertion order (the reference keeps edges in an unordered_multimap, NodeGraph.hpp:152, so its
  // instance order follows the hash function; a deterministic order is kept here so that packing is reproducible)
  const std::vector<Node*>& children() const { return mChildren; }
  void set_parent(Node& parent) {
    if (mParent == &parent) return;
    clear_parent();
    parent.mChildren.push_back(this);
    mParent = &parent;
  }
  void clear_parent() {
    if (!mParent) return;
    auto& c = mParent->mChildren;
    c.erase(std::remove(c.begin(), c.end(), this), c.end());
    mParent = nullptr;
  }
  Node& root() {
    Node* r = this;
    while (r->mParent) r = r->mParent;
    return *r;
  }
  Node& make_child(const std::string& name) {
    Node& n = mNodeGraph.emplace(name);
    n.set_parent(*this);
    return n;
  }

  // make_component<T>(args...): T(args...), T(Node*, args...) or T(Node&, args...), NodeGraph.hpp:247-268
  template <typename T, typename... Args>
  component_ptr<T> make_component(Args&&... args) {
    if (mComponents.count(typeid(T))) throw std::logic_error("Cannot make multiple components of the same type within the same node");
    auto it = mNodeGraph.mComponentMap.find(typeid(T));
    if (it == mNodeGraph.mComponentMap.end())
      it = mNodeGraph.mComponentMap.emplace(typeid(T), NodeGraph::component_map{[](const void* p) { delete reinterpret_cast<const T*>(p); }, {}}).first;
    T* ptr;
    if constexpr (std::is_constructible_v<T, Node&, Args...>)
      ptr = new T(*this, std::forward<Args>(args)...);
    else if constexpr (std::is_constructible_v<T, Node*, Args...>)
      ptr = new T(this, std::forward<Args>(args)...);
    else
      ptr = new T(std::forward<Args>(args)...);
    mComponents.emplace(typeid(T));
    it->second.mComponents[this] = ptr;
    return component_ptr<T>(this, ptr);
  }
  template <typename T>
  component_ptr<T> find() const {
    auto it = mNodeGraph.mComponentMap.find(typeid(T));
    if (it == mNodeGraph.mComponentMap.end()) return {};
    auto c = it->second.mComponents.find(this);
    return c == it->second.mComponents.end() ? component_ptr<T>() : component_ptr<T>(this, reinterpret_cast<T*>(c->second));
  }
  template <typename T>
  component_ptr<T> find_in_ancestor() const {
    for (const Node* n = this; n; n = n->mParent)
      if (auto c = n->find<T>()) return c;
    return {};
  }
  template <typename T>
  component_ptr<T> find_in_descendants() const {
    component_ptr<T> r;
    for_each_descendant<T>([&](const component_ptr<T>& c) {
      if (!r) r = c;
    });
    return r;
  }
  // breadth-first over this node and its descendants, NodeGraph.hpp:329-346
  template <typename T, typename F>
  void for_each_descendant(F&& fn) const {
    std::queue<const Node*> q;
    q.push(this);
    while (!q.empty()) {
      const Node* n = q.front();
      q.pop();
      if (auto c = n->find<T>()) fn(c);
      for (Node* c : n->children()) q.push(c);
    }
  }

 private:
  friend class NodeGraph;
  Node(NodeGraph& g, const std::string& name) : mNodeGraph(g), mName(name), mParent(nullptr) {}
  NodeGraph& mNodeGraph;
  std::string mName;
  Node* mParent;
  std::unordered_set<std::type_index> mComponents;
  std::vector<Node*> mChildren;
};

inline Node& NodeGraph::emplace(const std::string& name) {
  Node* ptr = new Node(*this, name);
  mNodes.emplace(ptr, std::unique_ptr<Node>(ptr));
  return *ptr;
}
inline void NodeGraph::erase(Node& node) {
  const std::vector<Node*> kids = node.children();
  for (Node* c : kids) c->clear_parent();
  node.clear_parent();
  mNodes.erase(&node);
}
inline NodeGraph::~NodeGraph() {
  for (auto& n : mNodes) {
    n.second->mParent = nullptr;
    n.second->mChildren.clear();
  }
  mNodes.clear();
}

// ------------------------------------------------------------------------------------------------
// vector / transform helpers (Common/hlsl_compat.hpp aliases Eigen; plain structs here)
// ------------------------------------------------------------------------------------------------
struct float2 {
  float x = 0, y = 0;
};
struct float3 {
  float x = 0, y = 0, z = 0;
  float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
  float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};
struct quatf {
  float3 xyz;
  float w = 1;
};
inline quatf quatf_identity() { return quatf{{0, 0, 0}, 1}; }
inline quatf angle_axis(float angle, float3 axis) {  // quatf.h:27-29
  const float s = std::sin(angle / 2);
  return quatf{{axis.x * s, axis.y * s, axis.z * s}, std::cos(angle / 2)};
}

using TransformData = sthip_TransformData;
using ProjectionData = sthip_ProjectionData;
using ViewData = sthip_ViewData;
using InstanceData = sthip_InstanceData;
using PackedVertexData = sthip_PackedVertexData;
using BDPTPushConstants = sthip_BDPTPushConstants;
using VisibilityInfo = sthip_VisibilityInfo;
using DepthInfo = sthip_DepthInfo;

// make_transform, transform.h:47-52: translation * rotation(quaternion) * scaling, the standard rotation matrix
// Eigen produces on the reference's host side
inline TransformData make_transform(float3 t, quatf r, float3 s) {
  TransformData o;
  const float sqw = r.w * r.w, sqx = r.xyz.x * r.xyz.x, sqy = r.xyz.y * r.xyz.y, sqz = r.xyz.z * r.xyz.z;
  const float invs = 1 / (sqx + sqy + sqz + sqw);
  float m[3][3];
  m[0][0] = (sqx - sqy - sqz + sqw) * invs;
  m[1][1] = (-sqx + sqy - sqz + sqw) * invs;
  m[2][2] = (-sqx - sqy + sqz + sqw) * invs;
  float tmp1 = r.xyz.x * r.xyz.y, tmp2 = r.xyz.z * r.w;
  m[1][0] = 2 * (tmp1 + tmp2) * invs;
  m[0][1] = 2 * (tmp1 - tmp2) * invs;
  tmp1 = r.xyz.x * r.xyz.z;
  tmp2 = r.xyz.y * r.w;
  m[2][0] = 2 * (tmp1 - tmp2) * invs;
  m[0][2] = 2 * (tmp1 + tmp2) * invs;
  tmp1 = r.xyz.y * r.xyz.z;
  tmp2 = r.xyz.x * r.w;
  m[2][1] = 2 * (tmp1 + tmp2) * invs;
  m[1][2] = 2 * (tmp1 - tmp2) * invs;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o.m[i][j] = m[i][j] * s[j];  // rotation * scaling
    o.m[i][3] = t[i];
  }
  return o;
}
inline TransformData transform_identity() { return make_transform({0, 0, 0}, quatf_identity(), {1, 1, 1}); }
// transform.h:88-104
inline TransformData tmul(const TransformData& a, const TransformData& b) {
  TransformData r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      float s = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
      if (j == 3) s += a.m[i][3];
      r.m[i][j] = s;
    }
  return r;
}
// TransformData::inverse(), transform.h:26-31: the reference takes Eigen's 4x4 inverse. Pinned here (and in
// stratum_amd/scene.py) as the adjugate of the 3x3 block over its determinant, evaluated in double in this
// exact order, then 0 - (inv * t); identity in, identity out.
inline TransformData inverse(const TransformData& t) {
  const double a00 = t.m[0][0], a01 = t.m[0][1], a02 = t.m[0][2];
  const double a10 = t.m[1][0], a11 = t.m[1][1], a12 = t.m[1][2];
  const double a20 = t.m[2][0], a21 = t.m[2][1], a22 = t.m[2][2];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double i00 = c00 / det, i01 = (a02 * a21 - a01 * a22) / det, i02 = (a01 * a12 - a02 * a11) / det;
  const double i10 = c01 / det, i11 = (a00 * a22 - a02 * a20) / det, i12 = (a02 * a10 - a00 * a12) / det;
  const double i20 = c02 / det, i21 = (a01 * a20 - a00 * a21) / det, i22 = (a00 * a11 - a01 * a10) / det;
  const double tx = t.m[0][3], ty = t.m[1][3], tz = t.m[2][3];
  TransformData r;
  r.m[0][0] = (float)i00, r.m[0][1] = (float)i01, r.m[0][2] = (float)i02, r.m[0][3] = (float)(0.0 - (i00 * tx + i01 * ty + i02 * tz));
  r.m[1][0] = (float)i10, r.m[1][1] = (float)i11, r.m[1][2] = (float)i12, r.m[1][3] = (float)(0.0 - (i10 * tx + i11 * ty + i12 * tz));
  r.m[2][0] = (float)i20, r.m[2][1] = (float)i21, r.m[2][2] = (float)i22, r.m[2][3] = (float)(0.0 - (i20 * tx + i21 * ty + i22 * tz));
  return r;
}
// transform.h:159-168
inline ProjectionData make_perspective(float fovy, float aspect, float2 offset, float znear) {
  ProjectionData r{};
  r.scale[1] = 1 / std::tan(fovy / 2);
  r.scale[0] = aspect * r.scale[1];
  r.offset[0] = offset.x;
  r.offset[1] = offset.y;
  r.near_plane = znear;
  r.far_plane = 0;
  r.vertical_fov = fovy;
  return r;
}
inline float3 back_project(const ProjectionData& p, float2 v) {  // transform.h:136-147
  float3 r;
  if (p.vertical_fov < 0) {
    r.x = (v.x - p.offset[0]) / p.scale[0];
    r.y = (v.y - p.offset[1]) / p.scale[1];
  } else {
    const float s = p.near_plane > 0 ? 1.f : (p.near_plane < 0 ? -1.f : 0.f);
    r.x = p.near_plane * (v.x * s - p.offset[0]) / p.scale[0];
    r.y = p.near_plane * (v.y * s - p.offset[1]) / p.scale[1];
  }
  r.z = p.near_plane;
  return r;
}

// node_to_world, Scene.cpp:108-117
inline TransformData node_to_world(const Node& node) {
  TransformData transform = transform_identity();
  for (const Node* p = &node; p != nullptr; p = p->parent())
    if (auto c = p->find<TransformData>()) transform = tmul(*c, transform);
  return transform;
}

// ------------------------------------------------------------------------------------------------
// scene components: Material.hpp:13-38, Scene.hpp:15-37
// ------------------------------------------------------------------------------------------------
// an RGBA32F texture (what the reference holds as an Image::View of a Texture2D<float4>), or an RGBA8_UNORM one
// (R8G8B8A8Unorm, Scene.cpp:178,229) when `bytes` is filled instead of `pixels`: it then goes up and stays resident as bytes
struct Image {
  uint32_t width = 0, height = 0;
  std::vector<float> pixels;   // width * height * 4, row 0 first
  std::vector<uint8_t> bytes;  // width * height * 4, row 0 first: a byte b is the texel (float)b / 255.0f (sthip.h)
  // An asset's image as its file holds it (sRGB, one to three channels, 16-bit, BC1-BC5: sthip_texel_format, from 16 up), when
  // `texels` is filled instead: a source of the material conversions, which decode it on the device. It is never resident:
  // Scene::decode_image makes the Image to bind (an emission image, a normal map).
  std::vector<uint8_t> texels;
  uint32_t texel_format = 0;
  bool is_raw() const { return !texels.empty(); }
  bool is_8bit() const { return !bytes.empty(); }
  float channel(size_t i) const { return is_8bit() ? (float)bytes[i] / 255.0f : pixels[i]; }
  // counts mark_dirty(): what tells the texels of one Image object apart. A host that repaints the texels in place (same extent,
  // same format) says so, and BDPT::update sends them to the resident scene (sthip_scene_set_images) instead of uploading.
  uint32_t serial = 0;
  void mark_dirty() { serial++; }
};
// a one-channel texture (Texture2D<float>): what Material::alpha_mask holds (R8Unorm coverage upstream, Scene.cpp:182), as floats
// or, when `bytes` is filled instead of `pixels`, as R8_UNORM
struct Image1 {
  uint32_t width = 0, height = 0;
  std::vector<float> pixels;   // width * height, row 0 first
  std::vector<uint8_t> bytes;  // width * height, row 0 first
  std::vector<uint8_t> texels;  // as Image::texels; a format of several channels gives its channel 0
  uint32_t texel_format = 0;
  bool is_raw() const { return !texels.empty(); }
  bool is_8bit() const { return !bytes.empty(); }
  uint32_t serial = 0;  // as Image::serial
  void mark_dirty() { serial++; }
};
// MaterialResources, image_value.h:34-66: images get their gImages / gImage1s index the first time a material stores them
struct MaterialResources {
  std::vector<const Image*> image4s;
  std::vector<const Image1*> image1s;
  uint32_t get_index(const component_ptr<Image1>& image) {
    if (!image) return ~0u;
    for (size_t i = 0; i < image1s.size(); i++)
      if (image1s[i] == image.get()) return (uint32_t)i;
    image1s.push_back(image.get());
    return (uint32_t)image1s.size() - 1;
  }
  std::vector<const std::vector<uint8_t>*> volumes;  // volume_data_map: NanoVDB buffers in first-use order (gVolumes)
  uint32_t get_index(const std::shared_ptr<std::vector<uint8_t>>& buffer) {  // image_value.h:49-55
    if (!buffer) return ~0u;
    for (size_t i = 0; i < volumes.size(); i++)
      if (volumes[i] == buffer.get()) return (uint32_t)i;
    volumes.push_back(buffer.get());
    return (uint32_t)volumes.size() - 1;
  }
  std::vector<std::pair<const std::vector<float>*, uint32_t>> distribution_data_map;  // table -> offset in gDistributions
  uint32_t distribution_data_size = 0;
  uint32_t get_index(const component_ptr<Image>& image) {
    if (!image) return ~0u;
    for (size_t i = 0; i < image4s.size(); i++)
      if (image4s[i] == image.get()) return (uint32_t)i;
    image4s.push_back(image.get());
    return (uint32_t)image4s.size() - 1;
  }
  uint32_t get_index(const std::vector<float>& data) {  // image_value.h:56-66
    for (const auto& e : distribution_data_map)
      if (e.first == &data) return e.second;
    const uint32_t r = distribution_data_size;
    distribution_data_map.emplace_back(&data, r);
    distribution_data_size += (uint32_t)data.size();
    return r;
  }
};
struct ImageValue4 {
  float value[4] = {0, 0, 0, 0};
  component_ptr<Image> image;  // null: constant value
};
// ImageValue1 / ImageValue3 (image_value.h): what the material conversions of Scene take (Scene.cpp:123-256). The image of an
// ImageValue3 is an rgba Image, as upstream's is a Texture2D<float4>
struct ImageValue1 {
  float value = 0;
  component_ptr<Image1> image;
};
struct ImageValue3 {
  float value[3] = {0, 0, 0};
  component_ptr<Image> image;
};
struct Material {
  ImageValue4 values[3];
  component_ptr<Image1> alpha_mask;  // Material.hpp:14
  component_ptr<Image> bump_image;
  float bump_strength = 1;
  // Material.hpp:15,19: the reduced minimum of the base colour's alpha, which only a converted material has
  bool has_min_alpha = false;
  uint32_t min_alpha = 0xFFFFFFFFu;
  bool alpha_test() const { return has_min_alpha && min_alpha < 0xFFFFFFFFu / 2; }
  float* base_color() { return values[0].value; }
  float& emission() { return values[0].value[3]; }
  float& metallic() { return values[1].value[0]; }
  float& roughness() { return values[1].value[1]; }
  float& anisotropic() { return values[1].value[2]; }
  float& subsurface() { return values[1].value[3]; }
  float& clearcoat() { return values[2].value[0]; }
  float& clearcoat_gloss() { return values[2].value[1]; }
  float& transmission() { return values[2].value[2]; }
  float& eta() { return values[2].value[3]; }
  // Material::store, Material.hpp:32-38
  void store(std::vector<uint32_t>& bytes, MaterialResources& resources) const {
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 4; j++) {
        uint32_t u;
        std::memcpy(&u, &values[i].value[j], 4);
        bytes.push_back(u);
      }
      bytes.push_back(resources.get_index(values[i].image));
    }
    bytes.push_back(resources.get_index(alpha_mask));
    bytes.push_back(resources.get_index(bump_image));
    uint32_t u;
    std::memcpy(&u, &bump_strength, 4);
    bytes.push_back(u);
  }
};
// what the reference's Mesh + copy_vertices produce for the path (positions, normals, uvs, indices)
struct Mesh {
  std::vector<float3> positions, normals;
  std::vector<float2> uvs;
  std::vector<uint32_t> indices;
  uint32_t index_stride = 4;  // 2 or 4 bytes
  // a rig over the mesh (MeshPrimitive::set_rig / set_pose): positions / normals above are its rest pose
  struct BlendTarget {
    std::vector<float3> positions, normals;
  };
  std::vector<BlendTarget> blend_targets;  // at most 4
  std::vector<sthip_VertexWeight> weights;  // one per vertex, or none (bone_count = 0)
  uint32_t bone_count = 0;
  bool posed = false;  // set_pose was called: until then the mesh is shown in its rest pose, bit for bit
  float blend_factors[4] = {0, 0, 0, 0};
  std::vector<TransformData> bones;
  bool rigged() const { return !blend_targets.empty() || bone_count; }
};
// One vertex of a rig in a pose, on the host: the arithmetic of sthip_scene_animate (include/sthip.h; compile with
// -ffp-contract=off), for a library that lacks the call and for drivers that upload posed meshes in full.
inline PackedVertexData pose_rig_vertex(PackedVertexData r, const PackedVertexData* const* targets, uint32_t target_count, size_t i, const float factors[4], const sthip_VertexWeight* weights,
                                        const TransformData* bones, uint32_t bone_count) {
  float p[3] = {r.position[0], r.position[1], r.position[2]}, n[3] = {r.normal[0], r.normal[1], r.normal[2]};
  if (target_count) {
    const float b[4] = {target_count > 0 ? factors[0] : 0.f, target_count > 1 ? factors[1] : 0.f, target_count > 2 ? factors[2] : 0.f, target_count > 3 ? factors[3] : 0.f};
    const float f = std::fmax(0.f, 1.f - (((std::fabs(b[0]) + std::fabs(b[1])) + std::fabs(b[2])) + std::fabs(b[3])));
    for (int a = 0; a < 3; a++) p[a] = f * p[a], n[a] = f * n[a];
    for (uint32_t k = 0; k < target_count; k++)
      for (int a = 0; a < 3; a++) {
        const float tp = b[k] * targets[k][i].position[a], tn = b[k] * targets[k][i].normal[a];
        p[a] = p[a] + tp;
        n[a] = n[a] + tn;
      }
    const float d0 = n[0] * n[0], d1 = n[1] * n[1], d2 = n[2] * n[2];
    const float inv = 1.0f / std::sqrt((d0 + d1) + d2);
    for (int a = 0; a < 3; a++) n[a] = n[a] * inv;
  }
  if (bone_count) {
    float m[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int j = 0; j < 4; j++)
      for (int row = 0; row < 3; row++)
        for (int c = 0; c < 4; c++) {
          const float t = bones[weights[i].indices[j]].m[row][c] * weights[i].weights[j];
          m[row][c] = m[row][c] + t;
        }
    float q[3], w[3];
    for (int row = 0; row < 3; row++) {
      const float a0 = m[row][0] * p[0], a1 = m[row][1] * p[1], a2 = m[row][2] * p[2];
      q[row] = ((a0 + a1) + a2) + m[row][3];
      const float c0 = m[row][0] * n[0], c1 = m[row][1] * n[1], c2 = m[row][2] * n[2];
      w[row] = (c0 + c1) + c2;
    }
    for (int a = 0; a < 3; a++) p[a] = q[a], n[a] = w[a];
  }
  for (int a = 0; a < 3; a++) r.position[a] = p[a], r.normal[a] = n[a];
  return r;
}
struct MeshPrimitive {
  component_ptr<Material> mMaterial;
  component_ptr<Mesh> mMesh;
  // A deforming mesh (skinning, cloth, a morph): new vertex data, the same indices. The scene is told with
  // Scene::mark_dirty() as after any other edit of the graph; BDPT::update then finds only vertex contents changed and
  // refits the resident tree (last_update_was_vertices_only()).
  void set_vertices(std::vector<float3> positions, std::vector<float3> normals = {}, std::vector<float2> uvs = {}) {
    if (!mMesh) throw std::invalid_argument("MeshPrimitive::set_vertices: no mesh");
    if (positions.size() != mMesh->positions.size()) throw std::invalid_argument("MeshPrimitive::set_vertices: the vertex count changed (topology must stay)");
    mMesh->positions = std::move(positions);
    if (!normals.empty()) mMesh->normals = std::move(normals);
    if (!uvs.empty()) mMesh->uvs = std::move(uvs);
  }
  // A rig over the mesh (kernels/anim.hlsl): up to 4 blend targets (positions and normals, one per vertex) and four bone
  // weights per vertex over bone_count bones (none: blend shapes only). The mesh's own vertices are the rest pose. With a
  // library that has sthip_scene_animate the rig goes to the device once after the next upload and set_pose then costs a
  // frame its bones and factors only (BDPT::update: last_update_was_vertices_only()); without it the host poses the mesh.
  void set_rig(std::vector<Mesh::BlendTarget> targets, std::vector<sthip_VertexWeight> weights = {}, uint32_t bone_count = 0) {
    if (!mMesh) throw std::invalid_argument("MeshPrimitive::set_rig: no mesh");
    const size_t n = mMesh->positions.size();
    if (targets.size() > 4) throw std::invalid_argument("MeshPrimitive::set_rig: more than 4 blend targets");
    for (const auto& t : targets)
      if (t.positions.size() != n || t.normals.size() != n) throw std::invalid_argument("MeshPrimitive::set_rig: a blend target has another vertex count than the mesh");
    if (bone_count > 1024) throw std::invalid_argument("MeshPrimitive::set_rig: more than 1024 bones");
    if ((bone_count != 0) != !weights.empty() || (bone_count && weights.size() != n)) throw std::invalid_argument("MeshPrimitive::set_rig: one weight record per vertex if and only if there are bones");
    for (const auto& w : weights)
      for (uint32_t index : w.indices)
        if (index >= bone_count) throw std::invalid_argument("MeshPrimitive::set_rig: a bone index is not below bone_count");
    mMesh->blend_targets = std::move(targets);
    mMesh->weights = std::move(weights);
    mMesh->bone_count = bone_count;
    mMesh->posed = false;
    mMesh->bones.clear();
  }
  // The pose of the rig: factors of the blend targets (absent ones ignored) and bone_count final matrices (the host has
  // applied hierarchy and keyframes). Scene::mark_dirty() tells the scene, as after any other edit.
  void set_pose(const std::array<float, 4>& factors, std::vector<TransformData> bones = {}) {
    if (!mMesh || !mMesh->rigged()) throw std::invalid_argument("MeshPrimitive::set_pose: the mesh has no rig");
    if (bones.size() != mMesh->bone_count) throw std::invalid_argument("MeshPrimitive::set_pose: the rig has another bone count");
    for (int k = 0; k < 4; k++) mMesh->blend_factors[k] = factors[k];
    mMesh->bones = std::move(bones);
    mMesh->posed = true;
  }
};
struct SpherePrimitive {  // Scene.hpp:34-37
  component_ptr<Material> mMaterial;
  float mRadius = 1;
};
// Material.hpp:72-87: a heterogeneous medium over NanoVDB float grids; the buffers are the bytes of a nanovdb::GridHandle
struct Medium {
  float density_scale[3] = {1, 1, 1};
  float anisotropy = 0;
  float albedo_scale[3] = {1, 1, 1};
  float attenuation_unit = 1;
  std::shared_ptr<std::vector<uint8_t>> density_buffer, albedo_buffer;
  // A dense box of densities in DEVICE memory as the source of the density grid (include/sthip.h: sthip_dense_volume_desc):
  // what a simulation leaves behind every frame. set_density_device() names it; the scene is then marked dirty as for any
  // change (Scene::mark_dirty()). Where nothing else changed, BDPT::update builds the grid on the device into the resident
  // scene (sthip_scene_set_volume); density_buffer, the host's copy, is then older than the device's and is fetched
  // (sthip_scene_read_volume) or built (sthip_build_volume) before it is uploaded anywhere. The memory must stay valid until
  // the BDPT::update that follows has returned. mark_density_dirty(): the bytes of density_buffer were rewritten in place.
  struct DenseSource {
    const float* dense = nullptr;
    uint32_t dims[3] = {0, 0, 0};
    int32_t origin[3] = {0, 0, 0};
    double voxel_size = 1;
    double translation[3] = {0, 0, 0};
    std::string name;
  };
  DenseSource dense_source;
  uint32_t density_serial = 0;               // counts set_density_device() / mark_density_dirty(): tells the grids of one buffer object apart
  mutable bool dense_pending = false;        // dense_source is newer than density_buffer AND than the resident grid
  mutable bool device_grid_newer = false;    // the resident grid (made from dense_source) is newer than density_buffer
  mutable bool has_device_world_bbox = false;
  mutable double device_world_bbox[6] = {0, 0, 0, 0, 0, 0};  // sthip_volume_info::world_bbox of that grid
  void set_density_device(const float* dense, const uint32_t dims[3], const int32_t origin[3], double voxel_size, const double translation[3], const char* name = "density") {
    dense_source.dense = dense;
    for (int a = 0; a < 3; a++) dense_source.dims[a] = dims[a], dense_source.origin[a] = origin[a], dense_source.translation[a] = translation[a];
    dense_source.voxel_size = voxel_size;
    dense_source.name = name ? name : "";
    if (!density_buffer) density_buffer = std::make_shared<std::vector<uint8_t>>();  // (the object the scene pools grids by)
    density_serial++;
    dense_pending = true;
    device_grid_newer = false;
  }
  void mark_density_dirty() {
    density_serial++;
    dense_pending = device_grid_newer = has_device_world_bbox = false;
  }
  sthip_dense_volume_desc dense_desc() const {
    sthip_dense_volume_desc d{};
    d.struct_size = sizeof(d);
    d.dense_is_device = 1;
    d.dense = dense_source.dense;
    for (int a = 0; a < 3; a++) d.dims[a] = dense_source.dims[a], d.origin[a] = dense_source.origin[a], d.translation[a] = dense_source.translation[a];
    d.voxel_size = dense_source.voxel_size;
    d.name = dense_source.name.c_str();
    return d;
  }
  // density_buffer is the current grid again: built from the pending dense source, or fetched from resident grid `index` of
  // `ctx` where BDPT::update installed it. Called before the buffer is uploaded (BDPT::update, every rank of MultiDeviceBDPT).
  void materialise(sthip_ctx* ctx, uint32_t index) const {
    if (dense_pending) {
      if (!sthip_build_volume) throw std::runtime_error("Medium: a dense device source needs a library with sthip_build_volume");
      const sthip_dense_volume_desc d = dense_desc();
      sthip_volume_info info{};
      (void)sthip_build_volume(ctx, &d, nullptr, 0, 0, &info);  // the size (refused: capacity 0)
      if (!info.bytes) throw std::runtime_error(std::string("sthip_build_volume: ") + sthip_last_error(ctx));
      density_buffer->resize((size_t)info.bytes);
      if (sthip_build_volume(ctx, &d, density_buffer->data(), info.bytes, 0, &info) != STHIP_OK) throw std::runtime_error(std::string("sthip_build_volume: ") + sthip_last_error(ctx));
    } else if (device_grid_newer) {
      uint64_t bytes = 0;
      (void)sthip_scene_read_volume(ctx, index, nullptr, 0, &bytes);
      density_buffer->resize((size_t)bytes);
      if (!bytes || sthip_scene_read_volume(ctx, index, density_buffer->data(), bytes, &bytes) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_read_volume: ") + sthip_last_error(ctx));
    }
    dense_pending = device_grid_newer = has_device_world_bbox = false;
  }
  void store(std::vector<uint32_t>& bytes, MaterialResources& pool) const {
    auto f = [&](float v) { uint32_t u; std::memcpy(&u, &v, 4); bytes.push_back(u); };
    for (float v : density_scale) f(v);
    f(anisotropy);
    for (float v : albedo_scale) f(v);
    f(attenuation_unit);
    bytes.push_back(pool.get_index(density_buffer));
    bytes.push_back(pool.get_index(albedo_buffer));
  }
  // GridData::mWorldBBox (6 doubles at byte 560 of the grid): what worldBBox() returns
  bool world_bbox(double box[6]) const {
    if (has_device_world_bbox) {
      std::memcpy(box, device_world_bbox, 48);
      return true;
    }
    if (!density_buffer || density_buffer->size() < 608) return false;
    std::memcpy(box, density_buffer->data() + 560, 48);
    return true;
  }
};

// dist2.h:80-154 build_distributions for a lat-long RGBA32F image: f(x, y) = luminance * sin(pi (y + 0.5) / H) is a
// double (float luminance times double sin), every running sum is stored as float, exactly as the reference's loops
inline void build_distributions(const Image& img, std::vector<float>& pdf_marginals, std::vector<float>& pdf_rows, std::vector<float>& cdf_marginals, std::vector<float>& cdf_rows) {
  const uint32_t W = img.width, H = img.height;
  pdf_marginals.assign(H, 0.f);
  pdf_rows.assign((size_t)W * H, 0.f);
  cdf_marginals.assign(H + 1, 0.f);
  cdf_rows.assign((size_t)(W + 1) * H, 0.f);
  const float invHeight = 1 / (float)H;
  auto f = [&](uint32_t x, uint32_t y) -> double {
    const size_t at = 4 * ((size_t)y * W + x);
    const float c[3] = {img.channel(at), img.channel(at + 1), img.channel(at + 2)};
    const float lum = (c[0] * 0.2126f + c[1] * 0.7152f) + c[2] * 0.0722f;
    return lum * std::sin(M_PI * (y + 0.5f) * invHeight);
  };
  for (uint32_t y = 0; y < H; y++) {
    float* row = &cdf_rows[(size_t)y * (W + 1)];
    row[0] = 0;
    for (uint32_t x = 0; x < W; x++) row[x + 1] = (float)(row[x] + f(x, y));
    const float integral = row[W];
    if (integral > 0) {
      for (uint32_t x = 0; x < W; x++) row[x] /= integral;
      for (uint32_t x = 0; x < W; x++) pdf_rows[(size_t)y * W + x] = (float)(f(x, y) / integral);
    } else {
      for (uint32_t x = 0; x < W; x++) {
        pdf_rows[(size_t)y * W + x] = float(1) / float(W);
        row[x] = float(x) / float(W);
      }
      row[W] = 1;
    }
  }
  cdf_marginals[0] = 0;
  for (uint32_t y = 0; y < H; y++) cdf_marginals[y + 1] = cdf_marginals[y] + cdf_rows[(size_t)y * (W + 1) + W];
  const float total_values = cdf_marginals[H];
  if (total_values > 0) {
    for (uint32_t y = 0; y < H; y++) cdf_marginals[y] /= total_values;
    cdf_marginals[H] = 1;
    for (uint32_t y = 0; y < H; y++) pdf_marginals[y] = cdf_rows[(size_t)y * (W + 1) + W] / total_values;
  } else {
    for (uint32_t y = 0; y < H; y++) {
      pdf_marginals[y] = float(1) / float(H);
      cdf_marginals[y] = float(y) / float(H);
    }
    cdf_marginals[H] = 1;
  }
  for (uint32_t y = 0; y < H; y++) cdf_rows[(size_t)y * (W + 1) + W] = 1;
}

// environment.h:8-25,96-150: constant radiance, or a lat-long image scaled by `value` with its sampling tables
struct Environment {
  float value[3] = {0, 0, 0};
  component_ptr<Image> image;
  std::vector<float> marginal_pdf, row_pdf, marginal_cdf, row_cdf;
  // true: the tables above are sized and zeroed, and the device builds them (sthip_scene_set_environment) after an upload and
  // after mark_image_dirty(). Where that cannot be — a library without the call, Scene::set_environment_on_device(false), the
  // multi-device driver — Scene::update has ensure_host_tables() build them here, as make_environment does without the flag.
  bool tables_on_device = false;
  uint32_t image_serial = 0;          // counts mark_image_dirty(): what tells the texels of one Image object apart
  uint32_t host_tables_serial = ~0u;  // the image_serial the tables above were built for on the host (~0u: never)
  bool is_zero() const { return value[0] == 0 && value[1] == 0 && value[2] == 0; }
  // A host that changes only these two things of a scene between frames (and marks the Scene dirty) gets
  // sthip_scene_set_environment from BDPT::update instead of an upload.
  void set_value(float r, float g, float b) { value[0] = r, value[1] = g, value[2] = b; }
  // The host wrote image->pixels (same extent). The host tables are NOT built again here: Scene::update builds them when it
  // packs for a library or a driver that cannot build them on the device, and otherwise packs them as they are and marks them
  // for the device (SceneData::mEnvironmentTablesOnDevice), which builds them in the environment-only call or after an upload.
  void mark_image_dirty() { image_serial++; }
  bool host_tables_current() const { return !image || (!tables_on_device && host_tables_serial == image_serial); }
  void ensure_host_tables() {
    if (!image || host_tables_serial == image_serial) return;
    build_distributions(*image, marginal_pdf, row_pdf, marginal_cdf, row_cdf);
    host_tables_serial = image_serial;
  }
  void store(std::vector<uint32_t>& bytes, MaterialResources& resources) const {
    for (int j = 0; j < 3; j++) {
      uint32_t u;
      std::memcpy(&u, &value[j], 4);
      bytes.push_back(u);
    }
    bytes.push_back(resources.get_index(image));
    if (image) {
      bytes.push_back(resources.get_index(marginal_pdf));
      bytes.push_back(resources.get_index(row_pdf));
      bytes.push_back(resources.get_index(marginal_cdf));
      bytes.push_back(resources.get_index(row_cdf));
    }
  }
};
// load_environment, environment.h:99-150, for an image that is already in memory
inline Environment make_environment(const component_ptr<Image>& image, float r = 1, float g = 1, float b = 1, bool tables_on_device = false) {
  Environment e;
  e.value[0] = r, e.value[1] = g, e.value[2] = b;
  e.image = image;
  e.tables_on_device = tables_on_device && image;
  if (e.tables_on_device) {
    const size_t W = image->width, H = image->height;
    e.marginal_pdf.assign(H, 0.f);
    e.row_pdf.assign(W * H, 0.f);
    e.marginal_cdf.assign(H + 1, 0.f);
    e.row_cdf.assign((W + 1) * H, 0.f);
  } else {
    e.ensure_host_tables();
  }
  return e;
}
struct Rect2D {
  int32_t x = 0, y = 0;
  uint32_t width = 0, height = 0;
};
struct Camera {
  ProjectionData mProjection{};
  Rect2D mImageRect;
  ViewData view() const {  // Scene.hpp:19-28
    ViewData v{};
    v.projection = mProjection;
    v.image_min[0] = mImageRect.x;
    v.image_min[1] = mImageRect.y;
    v.image_max[0] = mImageRect.x + (int32_t)mImageRect.width;
    v.image_max[1] = mImageRect.y + (int32_t)mImageRect.height;
    const float3 a = back_project(mProjection, {1, 1}), b = back_project(mProjection, {-1, -1});
    float ex = a.x - b.x, ey = a.y - b.y;
    if (mProjection.vertical_fov >= 0) {
      ex /= mProjection.near_plane;
      ey /= mProjection.near_plane;
    }
    v.projection.sensor_area = std::fabs(ex * ey);
    return v;
  }
};

// the HIP stream stands in for the Vulkan command buffer the reference threads through update()/render()
struct CommandBuffer {
  void* hip_stream = nullptr;
  sthip_ctx* ctx = nullptr;  // the device the material conversions of Scene run on (upstream: commandBuffer.mDevice); BDPT::context()
};

// Application.hpp:11-29: only the two events the renderer hooks
class Application {
 public:
  Node::Event<CommandBuffer&, float> OnUpdate;
  Node::Event<CommandBuffer&> OnRenderWindow;
  explicit Application(Node& node) : mNode(node) {}
  Node& node() const { return mNode; }
  void run_frame(CommandBuffer& cb, float dt = 0) {  // Application.cpp:64,69
    OnUpdate(cb, dt);
    OnRenderWindow(cb);
  }

 private:
  Node& mNode;
};

// ------------------------------------------------------------------------------------------------
// Scene: Scene.hpp:44-77, Scene::update Scene.cpp:299-684 (mesh instances only)
// ------------------------------------------------------------------------------------------------
class Scene {
 public:
  struct SceneData {
    std::vector<PackedVertexData> mVertices;
    std::vector<uint8_t> mIndices;
    std::vector<uint32_t> mMaterialData;
    std::vector<InstanceData> mInstances;
    std::vector<TransformData> mInstanceTransforms, mInstanceInverseTransforms, mInstanceMotionTransforms;
    std::vector<uint32_t> mLightInstanceMap;
    std::vector<Node*> mInstanceNodes;
    MaterialResources mResources;
    std::vector<sthip_image_desc> mImageDescs, mImage1Descs;
    // sthip_image_format per image: 1 where the descriptor points at the bytes of an 8-bit image. With a library that lacks
    // sthip_scene_upload_formats all are 0 and the 8-bit images are converted to floats here (mConvertedImages)
    std::vector<uint8_t> mImageFormats, mImage1Formats;
    std::vector<std::vector<float>> mConvertedImages;
    // the scene to a context, with the formats where some image is 8-bit
    int upload(sthip_ctx* ctx) const {
      const sthip_scene_desc d = desc();
      const auto any = [](const std::vector<uint8_t>& f) { return std::find_if(f.begin(), f.end(), [](uint8_t v) { return v != 0; }) != f.end(); };
      if (!any(mImageFormats) && !any(mImage1Formats)) return sthip_scene_upload(ctx, &d);
      return sthip_scene_upload_formats(ctx, &d, mImageFormats.empty() ? nullptr : mImageFormats.data(), mImage1Formats.empty() ? nullptr : mImage1Formats.data());
    }
    mutable std::vector<sthip_volume_desc> mVolumeDescs;                  // gVolumes (made again by desc(): a grid may have been materialised since)
    std::vector<uint32_t> mVolumeSerials;                                 // Medium::density_serial of the grids as they were packed, in gVolumes order
    std::vector<const Medium*> mVolumeMedia;                              // the Medium whose density grid gVolumes[i] is (nullptr: an albedo grid)
    std::vector<std::pair<const Medium*, uint32_t>> mMediumInstances;     // Medium component -> its volume instance (mInstanceTransformMap)
    std::vector<float> mDistributionData;  // gDistributions, Scene.cpp:670-683
    uint32_t mEnvironmentMaterialAddress = ~0u;
    // the environment as it was packed: its image object and that image's serial (Environment::mark_image_dirty), and whether
    // mDistributionData holds zeros where its tables go (the device builds them after the upload: BDPT::update)
    const Image* mEnvironmentImage = nullptr;
    uint32_t mEnvironmentImageSerial = 0;
    // Image::serial / Image1::serial of the images as they were packed, in gImages / gImage1s order
    std::vector<uint32_t> mImageSerials, mImage1Serials;
    bool mEnvironmentTablesOnDevice = false;
    uint32_t mMaterialCount = 0;
    uint32_t mEmissivePrimitiveCount = 0;
    // rigs posed on the device (Scene::pose_on_device()): mVertices holds their rest poses; mPoses[i] belongs to mRigs[i]
    struct Rig {
      uint32_t first_vertex = 0, vertex_count = 0, bone_count = 0;
      std::vector<std::vector<PackedVertexData>> targets;
      std::vector<sthip_VertexWeight> weights;
    };
    struct Pose {
      bool posed = false;
      float factors[4] = {0, 0, 0, 0};
      std::vector<TransformData> bones;
    };
    std::vector<Rig> mRigs;
    std::vector<Pose> mPoses;
    sthip_scene_desc desc() const {
      sthip_scene_desc d{};
      d.gVertices = mVertices.data();
      d.vertex_count = (uint32_t)mVertices.size();
      d.gIndices = mIndices.data();
      d.indices_bytes = (uint32_t)mIndices.size();
      d.gInstances = mInstances.data();
      d.instance_count = (uint32_t)mInstances.size();
      d.gInstanceTransforms = mInstanceTransforms.data();
      d.gInstanceInverseTransforms = mInstanceInverseTransforms.data();
      d.gInstanceMotionTransforms = mInstanceMotionTransforms.data();
      d.gMaterialData = mMaterialData.data();
      d.material_bytes = (uint32_t)(mMaterialData.size() * 4);
      d.gLightInstances = mLightInstanceMap.data();
      d.light_count = (uint32_t)mLightInstanceMap.size();
      d.gImages = mImageDescs.data();
      d.image_count = (uint32_t)mImageDescs.size();
      d.gImage1s = mImage1Descs.data();
      d.image1_count = (uint32_t)mImage1Descs.size();
      d.gDistributions = mDistributionData.empty() ? nullptr : mDistributionData.data();
      d.distribution_count = (uint32_t)mDistributionData.size();
      mVolumeDescs.clear();
      for (const auto* v : mResources.volumes) mVolumeDescs.push_back(sthip_volume_desc{v->data(), (uint64_t)v->size()});
      d.gVolumes = mVolumeDescs.empty() ? nullptr : mVolumeDescs.data();
      d.volume_count = (uint32_t)mVolumeDescs.size();
      return d;
    }
  };

  explicit Scene(Node& node) : mNode(node) {
    if (auto app = node.find_in_ancestor<Application>()) app->OnUpdate.add_listener(node, [this](CommandBuffer& cb, float dt) { update(cb, dt); }, Node::EventPriority::eDefault);
  }
  Node& node() const { return mNode; }
  const std::shared_ptr<SceneData>& data() const { return mSceneData; }
  void mark_dirty() { mDirty = true; }
  // true (the default with a library that has sthip_scene_animate): rigged meshes are packed in their rest pose with their
  // rigs beside them, and BDPT::update poses them on the device. false: update() below poses them on the host, and everything
  // downstream sees a deformed mesh like any other (the multi-device driver, which uploads deformed meshes in full).
  bool pose_on_device() const { return mPoseOnDevice; }
  void set_pose_on_device(bool on) {
    on = on && sthip_scene_set_rigs && sthip_scene_animate;
    if (on != mPoseOnDevice) mDirty = true;
    mPoseOnDevice = on;
  }

  // true (the default with a library that has sthip_scene_set_environment): BDPT::update sends a change of the environment
  // alone through that call, and an Environment with tables_on_device is packed with zeroed tables. false (what a library
  // without the call gets, and the multi-device driver sets): the tables are built here and every change is an upload.
  bool environment_on_device() const { return mEnvironmentOnDevice; }
  void set_environment_on_device(bool on) {
    on = on && sthip_scene_set_environment;
    if (on != mEnvironmentOnDevice) mDirty = true;
    mEnvironmentOnDevice = on;
  }
  // true: the transforms-only branch of BDPT::update has the device build the new top level (sthip_scene_set_transforms with
  // top_level = 1: a radix tree instead of the host's binned SAH — a cheaper call, a tree of somewhat lower quality, the same
  // frames). Off by default, and off for good with a library that lacks the call.
  bool top_level_on_device() const { return mTopLevelOnDevice; }
  void set_top_level_on_device(bool on) { mTopLevelOnDevice = on && sthip_scene_set_transforms; }

  // ---- the material conversions, Scene.cpp:123-256 -> kernels/material_convert.hlsl (sthip_convert_material) ----
  // The scalar part in binary32 as upstream writes it; with an image present the kernels run on cb.ctx (host form), and the
  // results become 8-bit Image / Image1 components on child nodes of this Scene's node. All given images must have one extent.
  static float luminance(const float c[3]) { return (c[0] * 0.2126f + c[1] * 0.7152f) + c[2] * 0.0722f; }
  ImageValue1 alpha_to_roughness(CommandBuffer& cb, const ImageValue1& alpha) { return to_roughness(cb, alpha, STHIP_CONVERT_ALPHA_TO_ROUGHNESS); }              // Scene.cpp:123-138
  ImageValue1 shininess_to_roughness(CommandBuffer& cb, const ImageValue1& shininess) { return to_roughness(cb, shininess, STHIP_CONVERT_SHININESS_TO_ROUGHNESS); }  // :139-154
  Material make_metallic_roughness_material(CommandBuffer& cb, const ImageValue3& base_color, const ImageValue4& metallic_roughness, const ImageValue3& transmission, float eta,
                                            const ImageValue3& emission) {  // Scene.cpp:156-203
    Material dst;
    if (emissive(cb, emission, dst)) return dst;
    for (int k = 0; k < 3; k++) dst.base_color()[k] = base_color.value[k];
    dst.emission() = 0;
    dst.metallic() = metallic_roughness.value[2];
    dst.roughness() = metallic_roughness.value[1];
    dst.anisotropic() = dst.subsurface() = dst.clearcoat() = 0;
    dst.clearcoat_gloss() = 1;
    dst.transmission() = luminance(transmission.value);
    dst.eta() = eta;
    convert(cb, STHIP_CONVERT_GLTF_PBR, base_color.image.get(), metallic_roughness.image.get(), transmission.image.get(), nullptr, dst);
    return dst;
  }
  Material make_diffuse_specular_material(CommandBuffer& cb, const ImageValue3& diffuse, const ImageValue3& specular, const ImageValue1& roughness, const ImageValue3& transmission, float eta,
                                          const ImageValue3& emission) {  // Scene.cpp:204-256
    Material dst;
    if (emissive(cb, emission, dst)) return dst;
    const float ld = luminance(diffuse.value), ls = luminance(specular.value), lt = luminance(transmission.value);
    const float den = (ld + ls) + lt;
    for (int k = 0; k < 3; k++) dst.base_color()[k] = ((diffuse.value[k] * ld + specular.value[k] * ls) + transmission.value[k] * lt) / den;
    dst.emission() = 0;
    dst.metallic() = ls / den;
    dst.roughness() = roughness.value;
    dst.anisotropic() = dst.subsurface() = dst.clearcoat() = 0;
    dst.clearcoat_gloss() = 1;
    dst.transmission() = lt / den;
    dst.eta() = eta;
    convert(cb, STHIP_CONVERT_DIFFUSE_SPECULAR, diffuse.image.get(), specular.image.get(), transmission.image.get(), roughness.image.get(), dst);
    return dst;
  }

  // Scene.cpp:299-684 for MeshPrimitive instances: same traversal order (breadth-first), same packing
  void update(CommandBuffer&, float) {
    if (!mDirty && mSceneData) return;
    // the previous frame's object-to-world transform of every instance's node (mInstanceTransformMap, Scene.cpp:398-427):
    // the motion transform is prev_object_to_world x world_to_object (make_instance_motion_transform, scene.h:49)
    std::unordered_map<const Node*, TransformData> prevTransforms;
    if (mSceneData)
      for (size_t i = 0; i < mSceneData->mInstanceNodes.size(); i++) prevTransforms.emplace(mSceneData->mInstanceNodes[i], mSceneData->mInstanceTransforms[i]);
    auto prev_of = [&](const Node& node, const TransformData& current) {
      auto it = prevTransforms.find(&node);
      return it == prevTransforms.end() ? current : it->second;
    };
    auto sd = std::make_shared<SceneData>();
    std::unordered_map<const Material*, uint32_t> materialMap;
    std::unordered_map<const Mesh*, std::pair<uint32_t, uint32_t>> meshMap;  // first_vertex, indices_byte_offset (shared by instances of one mesh)
    mNode.root().for_each_descendant<MeshPrimitive>([&](const component_ptr<MeshPrimitive>& prim) {
      if (!prim->mMesh || !prim->mMaterial) return;
      const Mesh& mesh = *prim->mMesh;
      // process_material, Scene.cpp:387-396
      auto mit = materialMap.find(prim->mMaterial.get());
      if (mit == materialMap.end()) {
        mit = materialMap.emplace(prim->mMaterial.get(), (uint32_t)(sd->mMaterialData.size() * sizeof(uint32_t))).first;
        prim->mMaterial->store(sd->mMaterialData, sd->mResources);
        sd->mMaterialCount++;
      }
      // copy_vertices + concatenation, copy_vertices.hlsl:29-37, Scene.cpp:461-485,643-658
      auto meshit = meshMap.find(&mesh);
      if (meshit == meshMap.end()) {
        meshit = meshMap.emplace(&mesh, std::make_pair((uint32_t)sd->mVertices.size(), (uint32_t)sd->mIndices.size())).first;
        for (size_t i = 0; i < mesh.positions.size(); i++) {
          PackedVertexData v{};
          v.position[0] = mesh.positions[i].x, v.position[1] = mesh.positions[i].y, v.position[2] = mesh.positions[i].z;
          if (i < mesh.normals.size()) v.normal[0] = mesh.normals[i].x, v.normal[1] = mesh.normals[i].y, v.normal[2] = mesh.normals[i].z;
          if (i < mesh.uvs.size()) v.u = mesh.uvs[i].x, v.v = mesh.uvs[i].y;
          sd->mVertices.push_back(v);
        }
        if (mesh.rigged() && (mPoseOnDevice || mesh.posed)) {
          const uint32_t first = meshit->second.first, count = (uint32_t)mesh.positions.size();
          SceneData::Rig rig;
          rig.first_vertex = first, rig.vertex_count = count, rig.bone_count = mesh.bone_count;
          for (const auto& t : mesh.blend_targets) {
            rig.targets.emplace_back(count, PackedVertexData{});
            for (uint32_t i = 0; i < count; i++) {
              PackedVertexData& v = rig.targets.back()[i];
              v.position[0] = t.positions[i].x, v.position[1] = t.positions[i].y, v.position[2] = t.positions[i].z;
              v.normal[0] = t.normals[i].x, v.normal[1] = t.normals[i].y, v.normal[2] = t.normals[i].z;
            }
          }
          rig.weights = mesh.weights;
          if (mPoseOnDevice) {
            SceneData::Pose pose;
            pose.posed = mesh.posed;
            std::memcpy(pose.factors, mesh.blend_factors, sizeof(pose.factors));
            pose.bones = mesh.bones;
            sd->mRigs.push_back(std::move(rig));
            sd->mPoses.push_back(std::move(pose));
          } else {  // posed here, with the arithmetic of the device's kernel
            const PackedVertexData* targets[4] = {nullptr, nullptr, nullptr, nullptr};
            for (size_t k = 0; k < rig.targets.size(); k++) targets[k] = rig.targets[k].data();
            for (uint32_t i = 0; i < count; i++)
              sd->mVertices[first + i] = pose_rig_vertex(sd->mVertices[first + i], targets, (uint32_t)rig.targets.size(), i, mesh.blend_factors, rig.weights.data(), mesh.bones.data(), rig.bone_count);
          }
        }
        for (uint32_t idx : mesh.indices) {
          if (mesh.index_stride == 2) {
            const uint16_t s = (uint16_t)idx;
            sd->mIndices.insert(sd->mIndices.end(), (const uint8_t*)&s, (const uint8_t*)&s + 2);
          } else {
            sd->mIndices.insert(sd->mIndices.end(), (const uint8_t*)&idx, (const uint8_t*)&idx + 4);
          }
        }
        while (sd->mIndices.size() & 3) sd->mIndices.push_back(0);  // align_up(size, 4), Scene.cpp:507
      }
      const uint32_t triCount = (uint32_t)(mesh.indices.size() / 3);
      if (triCount > 0xFFFF) throw std::invalid_argument("MeshPrimitive has more than 65535 triangles (16-bit primitive index, scene.h:23-24,37)");
      const TransformData transform = node_to_world(prim.node());
      // make_instance_triangles, scene.h:51-61; process_instance, Scene.cpp:398-427
      InstanceData inst{};
      inst.packed[0] = STHIP_INSTANCE_TYPE_TRIANGLES | (mit->second << 4);
      inst.packed[1] = 0xFFFu | (triCount << 12) | (mesh.index_stride << 28);
      inst.packed[2] = meshit->second.first;
      inst.packed[3] = meshit->second.second;
      const uint32_t instance_index = (uint32_t)sd->mInstances.size();
      if (prim->mMaterial->emission() > 0) {
        inst.packed[1] = (inst.packed[1] & ~0xFFFu) | ((uint32_t)sd->mLightInstanceMap.size() & 0xFFFu);
        sd->mLightInstanceMap.push_back(instance_index);
        sd->mEmissivePrimitiveCount += triCount;
      }
      sd->mInstances.push_back(inst);
      sd->mInstanceNodes.push_back(&prim.node());
      const TransformData inv = inverse(transform);
      sd->mInstanceTransforms.push_back(transform);
      sd->mInstanceInverseTransforms.push_back(inv);
      sd->mInstanceMotionTransforms.push_back(tmul(prev_of(prim.node(), transform), inv));  // make_instance_motion_transform(inv, prevObjectToWorld), scene.h:49
    });
    // sphere instances, Scene.cpp:511-553 (after every mesh instance)
    mNode.root().for_each_descendant<SpherePrimitive>([&](const component_ptr<SpherePrimitive>& prim) {
      if (!prim->mMaterial) return;
      auto mit = materialMap.find(prim->mMaterial.get());
      if (mit == materialMap.end()) {
        mit = materialMap.emplace(prim->mMaterial.get(), (uint32_t)(sd->mMaterialData.size() * sizeof(uint32_t))).first;
        prim->mMaterial->store(sd->mMaterialData, sd->mResources);
        sd->mMaterialCount++;
      }
      if (prim->mMaterial->emission() > 0) sd->mEmissivePrimitiveCount++;
      TransformData transform = node_to_world(prim.node());
      // :520-521: the radius is scaled by the DETERMINANT of the 3x3 block, the instance keeps only the translation
      const float(*m)[4] = transform.m;
      const float det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
      const float r = prim->mRadius * det;
      TransformData t{};
      t.m[0][0] = t.m[1][1] = t.m[2][2] = 1;
      t.m[0][3] = m[0][3], t.m[1][3] = m[1][3], t.m[2][3] = m[2][3];
      InstanceData inst{};  // make_instance_sphere, scene.h:62-70
      inst.packed[0] = STHIP_INSTANCE_TYPE_SPHERE | (mit->second << 4);
      inst.packed[1] = 0xFFFu;
      std::memcpy(&inst.packed[2], &r, 4);
      const uint32_t instance_index = (uint32_t)sd->mInstances.size();
      if (prim->mMaterial->emission() * (4 * M_PI * r * r) > 0) {
        inst.packed[1] = (inst.packed[1] & ~0xFFFu) | ((uint32_t)sd->mLightInstanceMap.size() & 0xFFFu);
        sd->mLightInstanceMap.push_back(instance_index);
      }
      sd->mInstances.push_back(inst);
      sd->mInstanceNodes.push_back(&prim.node());
      const TransformData inv = inverse(t);
      sd->mInstanceTransforms.push_back(t);
      sd->mInstanceInverseTransforms.push_back(inv);
      sd->mInstanceMotionTransforms.push_back(tmul(prev_of(prim.node(), t), inv));
    });
    // media, Scene.cpp:556-590 (after every sphere): one volume instance per Medium component
    mNode.root().for_each_descendant<Medium>([&](const component_ptr<Medium>& vol) {
      if (!vol || !vol->density_buffer) return;
      const uint32_t material_address = (uint32_t)(sd->mMaterialData.size() * sizeof(uint32_t));
      sd->mMaterialCount++;
      vol->store(sd->mMaterialData, sd->mResources);
      InstanceData inst{};  // make_instance_volume, scene.h:71-79
      inst.packed[0] = STHIP_INSTANCE_TYPE_VOLUME | (material_address << 4);
      inst.packed[1] = 0xFFFu;
      inst.packed[2] = sd->mResources.get_index(vol->density_buffer);
      sd->mVolumeSerials.resize(sd->mResources.volumes.size(), 0u);
      sd->mVolumeMedia.resize(sd->mResources.volumes.size(), nullptr);
      if (!sd->mVolumeMedia[inst.packed[2]]) sd->mVolumeSerials[inst.packed[2]] = vol->density_serial, sd->mVolumeMedia[inst.packed[2]] = vol.get();
      const TransformData transform = node_to_world(vol.node());
      sd->mMediumInstances.emplace_back(vol.get(), (uint32_t)sd->mInstances.size());
      sd->mInstances.push_back(inst);
      sd->mInstanceNodes.push_back(&vol.node());
      const TransformData inv = inverse(transform);
      sd->mInstanceTransforms.push_back(transform);
      sd->mInstanceInverseTransforms.push_back(inv);
      sd->mInstanceMotionTransforms.push_back(tmul(prev_of(vol.node(), transform), inv));
    });
    sd->mVolumeSerials.resize(sd->mResources.volumes.size(), 0u);
    sd->mVolumeMedia.resize(sd->mResources.volumes.size(), nullptr);
    // environment material, Scene.cpp:631-640: the first Environment whose value is not zero
    mNode.root().for_each_descendant<Environment>([&](const component_ptr<Environment>& environment) {
      if (environment && !environment->is_zero() && sd->mEnvironmentMaterialAddress == ~0u) {
        sd->mEnvironmentMaterialAddress = (uint32_t)(sd->mMaterialData.size() * sizeof(uint32_t));
        sd->mMaterialCount++;
        if (environment->image) {
          sd->mEnvironmentImage = environment->image.get();
          sd->mEnvironmentImageSerial = environment->image_serial;
          // the device builds the tables where it can and the host's are not there or not current (mark_image_dirty())
          sd->mEnvironmentTablesOnDevice = !environment->host_tables_current() && mEnvironmentOnDevice && environment->image->bytes.empty();
          if (!sd->mEnvironmentTablesOnDevice) {
            environment->ensure_host_tables();
            environment->tables_on_device = false;  // (they are real tables from here on)
          }
        }
        environment->store(sd->mMaterialData, sd->mResources);
      }
    });
    // an 8-bit image goes over as its bytes (sthip_scene_upload_formats); a library without the call gets the decoded floats
    const auto describe = [&](const std::vector<float>& pixels, const std::vector<uint8_t>& bytes, uint32_t width, uint32_t height, std::vector<sthip_image_desc>& descs, std::vector<uint8_t>& formats) {
      if (bytes.empty()) {
        descs.push_back(sthip_image_desc{pixels.data(), width, height});
        formats.push_back(0);
      } else if (sthip_scene_upload_formats) {
        descs.push_back(sthip_image_desc{reinterpret_cast<const float*>(bytes.data()), width, height});
        formats.push_back(1);
      } else {
        sd->mConvertedImages.emplace_back(bytes.size());
        std::vector<float>& f = sd->mConvertedImages.back();  // (its heap block stays where it is when the outer vector grows)
        for (size_t i = 0; i < bytes.size(); i++) f[i] = (float)bytes[i] / 255.0f;
        descs.push_back(sthip_image_desc{f.data(), width, height});
        formats.push_back(0);
      }
    };
    for (const Image* im : sd->mResources.image4s)
      if (im->is_raw()) throw std::invalid_argument("an Image of raw texels is a source, not a resident image: bind Scene::decode_image() of it");
    for (const Image1* im : sd->mResources.image1s)
      if (im->is_raw()) throw std::invalid_argument("an Image1 of raw texels is a source, not a resident image: bind Scene::decode_image1() of it");
    for (const Image* im : sd->mResources.image4s) describe(im->pixels, im->bytes, im->width, im->height, sd->mImageDescs, sd->mImageFormats);
    for (const Image1* im : sd->mResources.image1s) describe(im->pixels, im->bytes, im->width, im->height, sd->mImage1Descs, sd->mImage1Formats);
    for (const Image* im : sd->mResources.image4s) sd->mImageSerials.push_back(im->serial);
    for (const Image1* im : sd->mResources.image1s) sd->mImage1Serials.push_back(im->serial);
    sd->mDistributionData.resize(sd->mResources.distribution_data_size);
    for (const auto& e : sd->mResources.distribution_data_map) std::copy(e.first->begin(), e.first->end(), sd->mDistributionData.begin() + e.second);  // Scene.cpp:679-680
    mSceneData = sd;
    mDirty = false;
  }

 private:
  // the early return of both material functions, Scene.cpp:158-164,206-212
  bool emissive(CommandBuffer& cb, const ImageValue3& emission, Material& dst) {
    if (!(emission.value[0] > 0 || emission.value[1] > 0 || emission.value[2] > 0)) return false;
    const float l = luminance(emission.value);
    dst.values[0].image = (emission.image && emission.image->is_raw()) ? decode_image(cb, *emission.image) : emission.image;  // (bound as it is upstream: the sampler decodes)
    for (int k = 0; k < 3; k++) dst.base_color()[k] = emission.value[k] / l;
    dst.emission() = l;
    dst.eta() = 0;
    return true;
  }
  static sthip_ctx* convert_context(CommandBuffer& cb) {
    if (!sthip_convert_material) throw std::runtime_error("this libstratum_hip.so has no sthip_convert_material");
    if (!cb.ctx) throw std::invalid_argument("converting an image needs CommandBuffer::ctx (BDPT::context()): the kernels run on the device");
    return cb.ctx;
  }
  template <typename I>
  static void source(const I* im, uint32_t& width, uint32_t& height, const void*& p, uint8_t& format) {
    if (!im) return;
    if (!width) width = im->width, height = im->height;  // (upstream's order: the extent is the first present image's)
    if (im->width != width || im->height != height) throw std::invalid_argument("material conversion: all source images must have the extent of the first one");
    if (im->is_raw()) {
      if (im->texel_format < STHIP_TEXEL_FIRST) throw std::invalid_argument("material conversion: raw texels need a sthip_texel_format from 16 up");
      p = im->texels.data();
      format = (uint8_t)im->texel_format;
      return;
    }
    p = im->is_8bit() ? (const void*)im->bytes.data() : (const void*)im->pixels.data();
    format = im->is_8bit() ? 1 : 0;
  }
  // dst_channels 4 or 1 (channel 0); `identity`: the decode gives the source bytes back, so the result stays 8-bit
  template <typename I>
  static void decode_into(CommandBuffer& cb, const I& raw, uint32_t dst_channels, int resident, I& out) {
    if (!sthip_decode_texels) throw std::runtime_error("this libstratum_hip.so has no sthip_decode_texels");
    if (!cb.ctx) throw std::invalid_argument("decoding an image needs CommandBuffer::ctx (BDPT::context()): the kernel runs on the device");
    if (!raw.is_raw()) throw std::invalid_argument("decode_image: the image holds no raw texels");
    const bool identity = raw.texel_format >= STHIP_TEXEL_R8_UNORM && raw.texel_format <= STHIP_TEXEL_RGBA8_UNORM_;
    const bool as_bytes = resident < 0 ? identity : resident == 1;
    sthip_decode_texels_desc d{};
    d.src_format = raw.texel_format;
    d.width = raw.width, d.height = raw.height;
    d.dst_format = as_bytes ? 1 : 0;
    d.dst_channels = dst_channels;
    d.src = raw.texels.data();
    out.width = raw.width, out.height = raw.height;
    const size_t n = (size_t)raw.width * raw.height * dst_channels;
    if (as_bytes) {
      out.bytes.resize(n);
      d.dst = out.bytes.data();
    } else {
      out.pixels.resize(n);
      d.dst = out.pixels.data();
    }
    if (sthip_decode_texels(cb.ctx, &d) != STHIP_OK) throw std::runtime_error(std::string("sthip_decode_texels: ") + sthip_last_error(cb.ctx));
  }

 public:
  // An image of raw texels as the Image to bind where upstream binds the asset's image undecoded and lets the sampler decode it:
  // the emission image of an emissive material (Scene.cpp:158-164) and the normal map (load_gltf.cpp:104). RGBA8 / R8 where the
  // decode is the identity on bytes (unorm8 of any channel count), RGBA32F / R32F (exact) otherwise; `resident` 0 or 1 overrides.
  component_ptr<Image> decode_image(CommandBuffer& cb, const Image& raw, int resident = -1) {
    auto out = mNode.make_child("decoded image").make_component<Image>();
    decode_into(cb, raw, 4, resident, *out);
    return out;
  }
  component_ptr<Image1> decode_image1(CommandBuffer& cb, const Image1& raw, int resident = -1) {
    auto out = mNode.make_child("decoded image").make_component<Image1>();
    decode_into(cb, raw, 1, resident, *out);
    return out;
  }

 private:
  ImageValue1 to_roughness(CommandBuffer& cb, const ImageValue1& x, uint32_t kind) {
    ImageValue1 roughness;
    roughness.value = kind == STHIP_CONVERT_ALPHA_TO_ROUGHNESS ? std::sqrt(x.value) : std::sqrt(2.0f / (x.value + 2.0f));
    if (!x.image) return roughness;
    sthip_ctx* ctx = convert_context(cb);
    sthip_convert_material_desc d{};
    d.kind = kind;
    d.output_format = 1;
    source(x.image.get(), d.width, d.height, d.gInput, d.input_format);
    roughness.image = mNode.make_child("roughness").make_component<Image1>();
    roughness.image->width = d.width, roughness.image->height = d.height;
    roughness.image->bytes.resize((size_t)d.width * d.height);
    d.gRoughnessRW = roughness.image->bytes.data();
    if (sthip_convert_material(ctx, &d) != STHIP_OK) throw std::runtime_error(std::string("sthip_convert_material: ") + sthip_last_error(ctx));
    return roughness;
  }
  void convert(CommandBuffer& cb, uint32_t kind, const Image* diffuse, const Image* specular, const Image* transmittance, const Image1* roughness, Material& dst) {
    if (!diffuse && !specular && !transmittance && !roughness) return;
    sthip_ctx* ctx = convert_context(cb);
    sthip_convert_material_desc d{};
    d.kind = kind;
    d.output_format = 1;
    source(diffuse, d.width, d.height, d.gDiffuse, d.diffuse_format);
    source(specular, d.width, d.height, d.gSpecular, d.specular_format);
    source(transmittance, d.width, d.height, d.gTransmittance, d.transmittance_format);
    source(roughness, d.width, d.height, d.gRoughness, d.roughness_format);
    const size_t n = (size_t)d.width * d.height;
    for (int k = 0; k < 3; k++) {
      dst.values[k].image = mNode.make_child("material data").make_component<Image>();
      dst.values[k].image->width = d.width, dst.values[k].image->height = d.height;
      dst.values[k].image->bytes.resize(n * 4);
      d.gOutput[k] = dst.values[k].image->bytes.data();
    }
    std::vector<uint8_t> mask(diffuse ? n : 0);
    if (diffuse) d.gOutputAlphaMask = mask.data();
    dst.min_alpha = 0xFFFFFFFFu;
    d.gOutputMinAlpha = &dst.min_alpha;
    if (sthip_convert_material(ctx, &d) != STHIP_OK) throw std::runtime_error(std::string("sthip_convert_material: ") + sthip_last_error(ctx));
    dst.has_min_alpha = true;
    // upstream marks the geometry of a material whose alpha_test() is false opaque: its mask is never read, so it gets none
    if (diffuse && dst.alpha_test()) {
      dst.alpha_mask = mNode.make_child("alpha mask").make_component<Image1>();
      dst.alpha_mask->width = d.width, dst.alpha_mask->height = d.height;
      dst.alpha_mask->bytes = std::move(mask);
    }
  }
  Node& mNode;
  std::shared_ptr<SceneData> mSceneData;
  bool mDirty = true;
  bool mPoseOnDevice = sthip_scene_set_rigs && sthip_scene_animate;
  bool mEnvironmentOnDevice = sthip_scene_set_environment != nullptr;
  bool mTopLevelOnDevice = false;
};

// ------------------------------------------------------------------------------------------------
// Denoiser: Denoiser.hpp:9-60. The node BDPT::render hands its frame to when one is in the graph (BDPT.cpp:472-473,767-781):
// temporal accumulation (sthip_accumulate), then — with atrous_iterations() > 0 — the variance estimate, the filter passes and
// the history tap (sthip_denoise_filter). The state and its defaults are upstream's (Denoiser.cpp:73-77, Denoiser.hpp:56-57,
// gFilterKernelType = 1). The images live in host memory between frames, as the Frame's do (host form of both calls).
// Upstream's first frame, and one after reset_accumulation(), returns the radiance and accumulates nothing (Denoiser.cpp:267-271);
// here such a frame accumulates into an empty history — sample count 0 everywhere — as the Python host's does.
// gInstanceIndexMap is the identity: this host's Scene keeps an instance's index from frame to frame.
// ------------------------------------------------------------------------------------------------
class Denoiser {
 public:
  explicit Denoiser(Node& node) : mNode(node) {}
  Node& node() const { return mNode; }
  bool& reprojection() { return mReprojection; }
  bool& demodulate_albedo() { return mDemodulateAlbedo; }
  float& history_limit() { return mHistoryLimit; }                    // gHistoryLimit: "Target Sample Count"
  uint32_t& atrous_iterations() { return mAtrousIterations; }         // "Filter Iterations"
  uint32_t& filter_type() { return mFilterType; }                     // STHIP_FILTER_*
  uint32_t& history_tap() { return mHistoryTap; }                     // "History Tap Iteration"
  float& variance_boost_length() { return mVarianceBoostLength; }     // "Variance Boost Frames"
  float& sigma_luminance_boost() { return mSigmaLuminanceBoost; }
  void reset_accumulation() { mResetAccumulation = true; }
  uint32_t accumulated_frames() const { return mAccumulatedFrames; }

  // Denoiser::denoise (Denoiser.cpp:117-274). The colour images are RGBA32F, or RGBA16F when `half` (the context's
  // "half_color_precision"). Returns the image upstream returns — the accumulated colour, or gFilterImages[iterations % 2] —
  // which stays valid until the next call.
  const void* denoise(sthip_ctx* ctx, bool half, uint32_t width, uint32_t height, const void* radiance, const void* albedo, const std::vector<ViewData>& views,
                      const std::vector<VisibilityInfo>& visibility, const std::vector<DepthInfo>& depth, const std::vector<float>& prev_uvs) {
    const size_t n = (size_t)width * height, cb = half ? 8 : 16;
    if (mResetAccumulation || mWidth != width || mHeight != height || mHalf != half || mAccumColor.size() != n * cb) {
      mAccumColor.assign(n * cb, 0);
      mAccumMoments.assign(2 * n, 0.f);
      VisibilityInfo miss{};
      miss.instance_primitive_index = 0xFFFFFFFFu;
      mPrevVisibility.assign(n, miss);
      mPrevDepth.assign(n, DepthInfo{});
      mWidth = width, mHeight = height, mHalf = half;
      mResetAccumulation = false;
      mAccumulatedFrames = 0;
    }
    std::vector<uint8_t> color(n * cb, 0);
    std::vector<float> moments(2 * n, 0.f);
    sthip_accumulate_desc a{};
    a.width = width, a.height = height, a.view_count = (uint32_t)views.size();
    a.reprojection = mReprojection ? 1u : 0u, a.demodulate_albedo = mDemodulateAlbedo ? 1u : 0u;
    a.history_limit = mHistoryLimit;
    a.gViews = views.data();
    a.gRadiance = static_cast<const float*>(radiance), a.gAlbedo = static_cast<const float*>(albedo);
    a.gVisibility = visibility.data(), a.gDepth = depth.data(), a.gPrevUVs = prev_uvs.data();
    a.gPrevVisibility = mPrevVisibility.data(), a.gPrevDepth = mPrevDepth.data();
    a.gPrevAccumColor = reinterpret_cast<const float*>(mAccumColor.data()), a.gPrevAccumMoments = mAccumMoments.data();
    a.gAccumColor = reinterpret_cast<float*>(color.data()), a.gAccumMoments = moments.data();
    if (!sthip_accumulate) throw std::runtime_error("Denoiser::denoise: this libstratum_hip has no sthip_accumulate");
    if (sthip_accumulate(ctx, &a) != STHIP_OK) throw std::runtime_error(std::string("sthip_accumulate: ") + sthip_last_error(ctx));
    mAccumColor.swap(color);
    mAccumMoments.swap(moments);
    mPrevVisibility = visibility;
    mPrevDepth = depth;
    mAccumulatedFrames++;
    if (mAtrousIterations == 0) return mAccumColor.data();
    if (!sthip_denoise_filter) throw std::runtime_error("Denoiser::denoise: this libstratum_hip has no sthip_denoise_filter (filter iterations need it)");
    for (auto& f : mFilterImages) f.assign(n * cb, 0);
    sthip_denoise_desc d{};
    d.width = width, d.height = height, d.view_count = (uint32_t)views.size();
    d.iterations = mAtrousIterations, d.filter_type = mFilterType, d.history_tap = mHistoryTap;
    d.history_limit = mHistoryLimit;  // (one set of push constants serves both dispatches, Denoiser.cpp:225)
    d.variance_boost_length = mVarianceBoostLength, d.sigma_luminance_boost = mSigmaLuminanceBoost;
    d.gViews = views.data(), d.gVisibility = visibility.data(), d.gDepth = depth.data();
    d.gAccumColor = reinterpret_cast<float*>(mAccumColor.data());  // (the tapped colour is the history)
    d.gAccumMoments = mAccumMoments.data();
    d.gFilterImages[0] = reinterpret_cast<float*>(mFilterImages[0].data()), d.gFilterImages[1] = reinterpret_cast<float*>(mFilterImages[1].data());
    if (sthip_denoise_filter(ctx, &d) != STHIP_OK) throw std::runtime_error(std::string("sthip_denoise_filter: ") + sthip_last_error(ctx));
    return mFilterImages[mAtrousIterations % 2].data();
  }

 private:
  Node& mNode;
  bool mReprojection = true, mDemodulateAlbedo = true;  // Denoiser.cpp:76-77
  float mHistoryLimit = 0;                              // :73
  uint32_t mAtrousIterations = 0, mHistoryTap = 0;      // Denoiser.hpp:56-57
  uint32_t mFilterType = STHIP_FILTER_BOX3;             // atrous.hlsl:55,59
  float mVarianceBoostLength = 0, mSigmaLuminanceBoost = 3;  // Denoiser.cpp:75
  bool mResetAccumulation = false;
  uint32_t mAccumulatedFrames = 0;
  uint32_t mWidth = 0, mHeight = 0;
  bool mHalf = false;
  std::vector<uint8_t> mAccumColor, mFilterImages[2];
  std::vector<float> mAccumMoments;
  std::vector<VisibilityInfo> mPrevVisibility;
  std::vector<DepthInfo> mPrevDepth;
};

// ------------------------------------------------------------------------------------------------
// BDPT: BDPT.hpp:13-24. Errors surface as exceptions like in the reference (Shader.cpp:115, Instance.cpp:25).
// ------------------------------------------------------------------------------------------------
class BDPT {
 public:
  struct Frame {  // the outputs BDPT::render leaves in its FrameResources (BDPT.cpp:546-605)
    uint32_t width = 0, height = 0;
    std::vector<float> mRadiance, mAlbedo, mPrevUVs;
    std::vector<float> mTonemapResult;  // gOutput of the tone-map block, RGBA32F (BDPT.cpp:558)
    float mTonemapMax[4] = {0, 0, 0, 0};
    std::vector<VisibilityInfo> mVisibility;
    std::vector<DepthInfo> mDepth;
    uint64_t mRayCount[2] = {0, 0};
    std::vector<float> mDebugImage;  // gDebugImage (BDPT.cpp:560): RGBA32F, only with a debug mode
    // with set_half_color_precision(true) (mHalfColorPrecision, BDPT.cpp:231,553-558) these RGBA16F images (IEEE binary16 bits)
    // are filled instead of mRadiance / mAlbedo / mTonemapResult / mDebugImage, which then stay empty
    std::vector<uint16_t> mRadiance16, mAlbedo16, mTonemapResult16, mDebugImage16;
    // mDenoiseResult (BDPT.cpp:769): what the Denoiser returned and the tone map read; only with a Denoiser in the graph
    std::vector<float> mDenoiseResult;
    std::vector<uint16_t> mDenoiseResult16;
  };

  explicit BDPT(Node& node, int device = 0) : mNode(node) {
    if (sthip_create(device, &mCtx) != STHIP_OK) throw std::runtime_error(std::string("sthip_create: ") + sthip_last_error(nullptr));
    // one frame per call: the reservoir-reuse hash grids of a frame are the next frame's "previous" ones (BDPT.cpp:621-627)
    (void)sthip_set_option(mCtx, "reuse_grids_persist", 1);
    // BDPT.cpp:55-76
    mSamplingFlags = (1u << STHIP_eRemapThreads) | (1u << STHIP_eRayCones) | (1u << STHIP_eSampleBSDFs) | (1u << STHIP_eCoherentRR) | (1u << STHIP_eNormalMaps) |
                     (1u << STHIP_eNEE) | (1u << STHIP_eMIS) | (1u << STHIP_eDeferShadowRays);
    std::memset(&mPushConstants, 0, sizeof(mPushConstants));
    mPushConstants.gMinPathVertices = 4;
    mPushConstants.gMaxPathVertices = 8;
    mPushConstants.gMaxDiffuseVertices = 2;
    mPushConstants.gMaxNullCollisions = 64;
    mPushConstants.gEnvironmentSampleProbability = 0.5f;
    mPushConstants.gLightPresampleTileSize = 1024;
    mPushConstants.gLightPresampleTileCount = 128;
    mPushConstants.gLightPathCount = 64;
    mPushConstants.gReservoirM = 16;
    mPushConstants.gReservoirMaxM = 64;
    mPushConstants.gReservoirSpatialM = 4;
    mPushConstants.gHashGridBucketCount = 200000;
    mPushConstants.gHashGridMinBucketRadius = 0.1f;
    mPushConstants.gHashGridBucketPixelRadius = 6;
    if (auto app = node.find_in_ancestor<Application>())
      app->OnUpdate.add_listener(node, [this](CommandBuffer& cb, float dt) { update(cb, dt); }, Node::EventPriority::eAlmostLast);  // BDPT.cpp:38
  }
  virtual ~BDPT() {
    mAsync.reset();  // (the pinned ring of submit(), through the deleter submit() installed: before the context goes)
    sthip_destroy(mCtx);
  }
  BDPT(const BDPT&) = delete;
  sthip_ctx* context() const { return mCtx; }  // for CommandBuffer::ctx

  // the instance arguments BDPT's constructor reads (BDPT.cpp:78-127): `minPathVertices`, `maxPathVertices`,
  // `maxDiffuseVertices`, `maxNullCollisions`, `environmentSampleProbability`, `lightPresampleTileSize`,
  // `lightPresampleTileCount`, and `bdptFlag` = [~|!]name with the flag's display name lower-cased, spaces removed
  void set_argument(const std::string& key, const std::string& value) {
    if (key == "bdptFlag") return set_flag(value);
    if (key == "environmentSampleProbability") {
      mPushConstants.gEnvironmentSampleProbability = std::stof(value);
      return;
    }
    static const std::pair<const char*, uint32_t BDPTPushConstants::*> fields[] = {
        {"minPathVertices", &BDPTPushConstants::gMinPathVertices},
        {"maxPathVertices", &BDPTPushConstants::gMaxPathVertices},
        {"maxDiffuseVertices", &BDPTPushConstants::gMaxDiffuseVertices},
        {"maxNullCollisions", &BDPTPushConstants::gMaxNullCollisions},
        {"lightPresampleTileSize", &BDPTPushConstants::gLightPresampleTileSize},
        {"lightPresampleTileCount", &BDPTPushConstants::gLightPresampleTileCount},
        {"lightPathCount", &BDPTPushConstants::gLightPathCount},
        {"reservoirM", &BDPTPushConstants::gReservoirM},
        {"reservoirMaxM", &BDPTPushConstants::gReservoirMaxM},
        {"reservoirSpatialM", &BDPTPushConstants::gReservoirSpatialM},
        {"hashGridBucketCount", &BDPTPushConstants::gHashGridBucketCount},
    };
    for (const auto& f : fields)
      if (key == f.first) mPushConstants.*(f.second) = (uint32_t)std::stoul(value);
  }
  void set_flag(std::string arg) {
    if (arg.empty()) return;
    bool on = true;
    if (arg[0] == '~' || arg[0] == '!') {
      on = false;
      arg = arg.substr(1);
    }
    for (char& c : arg) c = (char)std::tolower((unsigned char)c);
    static const char* names[STHIP_eBDPTFlagCount] = {
        "performancecounters", "remapthreads", "coherentrr", "coherentsampling", "fliptriangleuvs", "flipnormalmaps", "alphatest", "normalmaps",
        "shadingnormalshadowfix", "raycones", "samplebsdfs", "nee", "neereservoirs", "neereservoirreuse", "mis", "samplelightpower",
        "uniformspheresampling", "presamplelights", "defershadowrays", "connecttoviews", "connecttolightpaths", "lightvertexcache", "lvcreservoirs",
        "lvcreservoirreuse", "jitterhashgridlookups", "sampleenvironmentmapdirectly"};
    for (uint32_t i = 0; i < STHIP_eBDPTFlagCount; i++)
      if (arg == names[i]) {  // unknown names are ignored, as upstream
        if (on)
          mSamplingFlags |= 1u << i;
        else
          mSamplingFlags &= ~(1u << i);
      }
  }

  Node& node() const { return mNode; }
  uint32_t& sampling_flags() { return mSamplingFlags; }
  BDPTPushConstants& push_constants() { return mPushConstants; }
  const Frame& prev_result() const { return mPrevFrame; }  // BDPT.hpp:18
  bool last_update_was_transforms_only() const { return mLastUpdateWasTransformsOnly; }
  // Instance matrices that lie in device memory (rigid bodies, particles, a crowd simulated there) go to the resident scene
  // without a copy to the host (sthip_scene_set_transforms with device_ptr = 1 and the device-built top level): `xf` =
  // instance_count sthip_TransformData records readable in the order of the context's stream; `inv` NULL: derived by the
  // library with transform_inverse's arithmetic; `motion` NULL: the identity, or with derive_motion previous x inverse.
  // The bound Scene's own matrices do not follow (sthip_scene_read_transforms says what is resident); its next change is
  // compared against what it held before. Throws on a refusal, a moved instance of the merged mesh without a kept scene included.
  void set_instance_transforms_device(const void* xf, const void* inv, const void* motion, bool derive_motion) {
    if (!sthip_scene_set_transforms) throw std::runtime_error("set_instance_transforms_device: the library lacks sthip_scene_set_transforms");
    if (!mBoundData) throw std::runtime_error("set_instance_transforms_device: no scene is bound");
    sthip_transforms_desc t{};
    t.transforms = static_cast<const sthip_TransformData*>(xf);
    t.inverse_transforms = static_cast<const sthip_TransformData*>(inv);
    t.motion_transforms = static_cast<const sthip_TransformData*>(motion);
    t.instance_count = (uint32_t)mBoundData->mInstanceTransforms.size();
    t.device_ptr = 1;
    t.top_level = 1;
    t.derive_motion = derive_motion ? 1u : 0u;
    if (sthip_scene_set_transforms(mCtx, &t, sizeof(t), nullptr) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_set_transforms: ") + sthip_last_error(mCtx));
  }
  // Vertices that lie in device memory (a cloth or soft-body step there) go to the resident scene without a copy to the host
  // (sthip_scene_set_vertices with device_ptr = 1): `positions` (required), `normals` and `texcoords` (NULL: the resident
  // fields stay) are strided streams of vertex_count elements readable in the order of the context's stream;
  // recompute_normals: the shading normals of the range are made on the device from the moved positions (normals NULL).
  // The bound Scene's own vertices do not follow (sthip_scene_read_vertices says what is resident): they are marked as behind
  // the device, and the next update() that binds new SceneData uploads it instead of comparing against them. Throws on a
  // refusal and on a layout the library does not refit without a kept scene.
  void set_vertices_device(uint32_t first_vertex, uint32_t vertex_count, const void* positions, uint32_t position_stride, const void* normals = nullptr, uint32_t normal_stride = 0,
                           const void* texcoords = nullptr, uint32_t texcoord_stride = 0, bool recompute_normals = false, sthip_refit_info* info = nullptr) {
    if (!sthip_scene_set_vertices) throw std::runtime_error("set_vertices_device: the library lacks sthip_scene_set_vertices");
    if (!mBoundData) throw std::runtime_error("set_vertices_device: no scene is bound");
    sthip_vertex_streams s{};
    s.struct_size = sizeof(s);
    s.first_vertex = first_vertex;
    s.vertex_count = vertex_count;
    s.device_ptr = 1;
    s.recompute_normals = recompute_normals ? 1u : 0u;
    s.position_stride = position_stride;
    s.normal_stride = normal_stride;
    s.texcoord_stride = texcoord_stride;
    s.positions = positions;
    s.normals = normals;
    s.texcoords = texcoords;
    if (sthip_scene_set_vertices(mCtx, &s, info) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_set_vertices: ") + sthip_last_error(mCtx));
    if (vertex_count) mVerticesBehindDevice = true;
  }
  bool vertices_behind_device() const { return mVerticesBehindDevice; }
  bool last_update_was_vertices_only() const { return mLastUpdateWasVerticesOnly; }  // (no transform changed with them)
  bool last_update_was_environment_only() const { return mLastUpdateWasEnvironmentOnly; }
  bool last_update_was_materials_only() const { return mLastUpdateWasMaterialsOnly; }
  bool last_update_was_volumes_only() const { return mLastUpdateWasVolumesOnly; }
  // sthip_scene_set_volume for a grid that is the only change (default: on where the library has the call); off: such a
  // change is an upload, as with a library without the symbol
  void set_volumes_on_device(bool on) { mVolumesOnDevice = on; }
  uint32_t volume_calls() const { return mVolumeCalls; }                    // sthip_scene_set_volume calls of update() so far
  uint32_t material_data_calls() const { return mMaterialDataCalls; }       // sthip_scene_set_material_data calls of update() so far
  uint32_t image_calls() const { return mImageCalls; }                      // sthip_scene_set_images calls of update() so far
  uint32_t upload_calls() const { return mUploadCalls; }                    // sthip_scene_upload(_formats) calls of update() so far
  uint32_t environment_calls() const { return mEnvironmentCalls; }          // sthip_scene_set_environment calls of update() so far
  // tone-map state the reference keeps on its pipeline objects (BDPT.cpp:44-54,190-193,304-309)
  uint32_t& tonemap_mode() { return mTonemapMode; }
  float& exposure() { return mExposure; }
  float& exposure_alpha() { return mExposureAlpha; }
  bool& gamma_correction() { return mGammaCorrection; }
  // "Export" -> "Save" (BDPT.cpp:313-337): the last frame's radiance as a Radiance .hdr file
  // (a half frame is upcast exactly, det_f16tof32: the writer takes RGBA32F)
  void export_hdr(const std::string& path) const {
    if (mPrevFrame.mRadiance.empty() && mPrevFrame.mRadiance16.empty()) throw std::runtime_error("BDPT::export_hdr: no frame rendered yet");
    std::vector<float> up;
    if (mPrevFrame.mRadiance.empty()) {
      up.resize(mPrevFrame.mRadiance16.size());
      for (size_t i = 0; i < up.size(); i++) up[i] = det_f16tof32(mPrevFrame.mRadiance16[i]);
    }
    if (sthip_write_hdr(path.c_str(), mPrevFrame.width, mPrevFrame.height, up.empty() ? mPrevFrame.mRadiance.data() : up.data()) != STHIP_OK)
      throw std::runtime_error("BDPT::export_hdr: cannot write " + path);
  }
  // the inspector's "Half precision" (BDPT.cpp:231, mHalfColorPrecision): radiance, albedo, debug and tone-map images in RGBA16F
  // (include/sthip.h "half_color_precision"); a change drops the persisted debug image, as a change of the debug mode does
  virtual void set_half_color_precision(bool on) {
    if (sthip_set_option(mCtx, "half_color_precision", on ? 1 : 0) != STHIP_OK) throw std::runtime_error(std::string("half_color_precision: ") + sthip_last_error(mCtx));
    if (on != mHalfColorPrecision) {
      mDebugImage.clear();
      mDebugImage16.clear();
    }
    mHalfColorPrecision = on;
  }
  bool half_color_precision() const { return mHalfColorPrecision; }

  // BDPT::update (BDPT.cpp:341-421): (re)bind the scene when Scene::update produced new SceneData
  virtual void update(CommandBuffer& cb, float) {
    auto scene = mNode.find_in_ancestor<Scene>();
    if (!scene) scene = mNode.root().find_in_descendants<Scene>();
    if (!scene || !scene->data() || scene->data().get() == mBound) return;
    (void)sthip_set_stream(mCtx, cb.hip_stream);
    const sthip_scene_desc d = scene->data()->desc();
    // Only instances moved since the bound SceneData (same geometry, materials, images, volumes): the bottom levels in HBM
    // are still right, as the reference's cached BLASes are (Scene.cpp:435-459); rebuild the top level only.
    bool updated = false;
    mLastUpdateWasVerticesOnly = false;
    mLastUpdateWasEnvironmentOnly = false;
    mLastUpdateWasMaterialsOnly = false;
    const Scene::SceneData& sd = *scene->data();
    const bool rigs = !sd.mRigs.empty();  // (packed only with a library that has the calls: Scene::pose_on_device())
    mLastUpdateWasVolumesOnly = false;
    if (mVerticesBehindDevice) {
      // set_vertices_device wrote the resident vertices: the bound data's are older than the device's, and a comparison
      // against them would take a mesh for unchanged that is not. The new data is uploaded whole.
      mBoundData = nullptr;  // (every partial path below needs it)
      mVerticesBehindDevice = false;
    }
    if (mBoundData && !same_volume_serials(*mBoundData, sd)) {
      // A density grid changed (Medium::set_density_device / mark_density_dirty). Where it is the only change, the grid is
      // replaced in the resident scene: built there from the dense device source, or copied from the host's bytes. Otherwise,
      // with a library without the call, under MultiDeviceBDPT (mVolumesOnDevice = false) or where the library refuses:
      // the grids are made current on the host and the scene is uploaded; no partial update may pass over a changed grid.
      if (mVolumesOnDevice && sthip_scene_set_volume && volumes_only_changed(*mBoundData, sd) && set_volumes(*mBoundData, sd) == STHIP_OK) {
        mLastUpdateWasVolumesOnly = true;
        mLastUpdateWasTransformsOnly = false;
        mBound = scene->data().get();
        mBoundData = scene->data();
        return;
      }
      mBoundData = nullptr;  // (every partial path below needs it)
    }
    if (scene->environment_on_device() && mBoundData && environment_only_changed(*mBoundData, sd)) {
      // Only the environment's value and / or the texels of its image changed: the value, the texels, the mip chain and the
      // tables are replaced in the resident scene. A call the library refuses as unsupported (an image a material shares): upload.
      const int rc = set_environment(*mBoundData, sd);
      if (rc == STHIP_OK) {
        mLastUpdateWasEnvironmentOnly = true;
        mLastUpdateWasTransformsOnly = false;
        mBound = scene->data().get();
        mBoundData = scene->data();
        return;
      }
    }
    if (mMaterialsOnDevice && sthip_scene_set_images && sthip_scene_set_material_data && mBoundData && materials_only_changed(*mBoundData, sd)) {
      // Only bytes of gMaterialData and / or the texels of images at the same extents changed (an inspector's colour, a
      // repainted texture): the differing byte range and the differing images go to the resident scene, which makes the mip
      // chains, the image ranges and the material analysis again. An edit the library refuses as unsupported (a light that goes
      // out, a mask that a triangle instance gains): upload.
      const int rc = set_materials(*mBoundData, sd);
      if (rc == STHIP_OK) {
        mLastUpdateWasMaterialsOnly = true;
        mLastUpdateWasTransformsOnly = false;
        mBound = scene->data().get();
        mBoundData = scene->data();
        return;
      }
    }
    if (rigs && mRigsResident && mBoundData && same_geometry(*mBoundData, sd) && !same_poses(*mBoundData, sd)) {
      // Only poses changed (and perhaps transforms): the rigs are resident, the bones and factors go to the device and the
      // meshes are posed and the tree refitted there. A layout the library cannot serve without a kept scene answers UNSUPPORTED: upload.
      const bool moved = !same_bytes(mBoundData->mInstanceTransforms, sd.mInstanceTransforms) || !same_bytes(mBoundData->mInstanceInverseTransforms, sd.mInstanceInverseTransforms) ||
                         !same_bytes(mBoundData->mInstanceMotionTransforms, sd.mInstanceMotionTransforms);
      int rc = animate(sd);
      if (rc == STHIP_OK && moved) {
        rc = sthip_scene_update_transforms(mCtx, d.gInstanceTransforms, d.gInstanceInverseTransforms, d.gInstanceMotionTransforms, d.instance_count);
        if (rc != STHIP_OK && rc != STHIP_ERR_UNSUPPORTED) throw std::runtime_error(std::string("sthip_scene_update_transforms: ") + sthip_last_error(mCtx));
      }
      if (rc == STHIP_OK) {
        mLastUpdateWasVerticesOnly = !moved;
        mLastUpdateWasTransformsOnly = false;
        mBound = scene->data().get();
        mBoundData = scene->data();
        mPushConstants.gLightCount = d.light_count;
        mPushConstants.gEnvironmentMaterialAddress = sd.mEnvironmentMaterialAddress;
        return;
      }
    } else if (mBoundData && same_geometry(*mBoundData, *scene->data()) && (!rigs || (mRigsResident && same_poses(*mBoundData, sd)))) {
      int rc;
      if (scene->top_level_on_device() && sthip_scene_set_transforms) {  // Scene::set_top_level_on_device: the same matrices, the top level built on the device
        sthip_transforms_desc t{};
        t.transforms = d.gInstanceTransforms;
        t.inverse_transforms = d.gInstanceInverseTransforms;
        t.motion_transforms = d.gInstanceMotionTransforms;
        t.instance_count = d.instance_count;
        t.top_level = 1;
        rc = sthip_scene_set_transforms(mCtx, &t, sizeof(t), nullptr);
      } else {
        rc = sthip_scene_update_transforms(mCtx, d.gInstanceTransforms, d.gInstanceInverseTransforms, d.gInstanceMotionTransforms, d.instance_count);
      }
      if (rc == STHIP_OK)
        updated = true;
      else if (rc != STHIP_ERR_UNSUPPORTED)
        throw std::runtime_error(std::string("sthip_scene_update_transforms: ") + sthip_last_error(mCtx));
    } else if (mRefitDeformedMeshes && mBoundData && sthip_scene_update_vertices && !rigs && same_topology(*mBoundData, *scene->data())) {  // (a new rest pose of a rig: an upload)
      // A mesh deformed (same indices, instances, materials; only the contents of gVertices differ): the range that changed
      // goes to the device and the resident bottom levels are refitted there (the reference rebuilds the BLAS of a dirty mesh,
      // Scene.cpp:345,435-459). A layout the library does not refit without a kept scene answers UNSUPPORTED: upload.
      const auto& a = mBoundData->mVertices;
      const auto& b = scene->data()->mVertices;
      size_t lo = 0, hi = b.size();
      while (lo < hi && !std::memcmp(&a[lo], &b[lo], sizeof(PackedVertexData))) lo++;
      while (hi > lo && !std::memcmp(&a[hi - 1], &b[hi - 1], sizeof(PackedVertexData))) hi--;
      const bool moved = !same_bytes(mBoundData->mInstanceTransforms, scene->data()->mInstanceTransforms) ||
                         !same_bytes(mBoundData->mInstanceInverseTransforms, scene->data()->mInstanceInverseTransforms) ||
                         !same_bytes(mBoundData->mInstanceMotionTransforms, scene->data()->mInstanceMotionTransforms);
      int rc = sthip_scene_update_vertices(mCtx, b.data() + lo, (uint32_t)lo, (uint32_t)(hi - lo), nullptr);
      if (rc != STHIP_OK && rc != STHIP_ERR_UNSUPPORTED) throw std::runtime_error(std::string("sthip_scene_update_vertices: ") + sthip_last_error(mCtx));
      if (rc == STHIP_OK && moved) {  // instances moved as well: the top level once more, over the refitted bottom levels
        rc = sthip_scene_update_transforms(mCtx, d.gInstanceTransforms, d.gInstanceInverseTransforms, d.gInstanceMotionTransforms, d.instance_count);
        if (rc != STHIP_OK && rc != STHIP_ERR_UNSUPPORTED) throw std::runtime_error(std::string("sthip_scene_update_transforms: ") + sthip_last_error(mCtx));
      }
      if (rc == STHIP_OK) {
        mLastUpdateWasVerticesOnly = !moved;
        mLastUpdateWasTransformsOnly = false;
        mBound = scene->data().get();
        mBoundData = scene->data();
        mPushConstants.gLightCount = d.light_count;
        mPushConstants.gEnvironmentMaterialAddress = scene->data()->mEnvironmentMaterialAddress;
        return;
      }
    }
    mLastUpdateWasTransformsOnly = updated;
    if (!updated)  // the host's grids must be the current ones: a dense source not built yet, a grid only the device has
      for (size_t i = 0; i < sd.mVolumeMedia.size(); i++)
        if (sd.mVolumeMedia[i] && (sd.mVolumeMedia[i]->dense_pending || sd.mVolumeMedia[i]->device_grid_newer)) sd.mVolumeMedia[i]->materialise(mCtx, (uint32_t)i);
    if (!updated && sd.upload(mCtx) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_upload: ") + sthip_last_error(mCtx));
    if (!updated) mUploadCalls++;
    if (!updated && sd.mEnvironmentTablesOnDevice) {  // zeroed tables went up: the device builds them from the resident texels
      sthip_environment_desc e{};
      e.struct_size = sizeof(e);
      e.material_address = sd.mEnvironmentMaterialAddress;
      mEnvironmentCalls++;
      if (sthip_scene_set_environment(mCtx, &e, nullptr) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_set_environment: ") + sthip_last_error(mCtx));
    }
    if (!updated) {  // the upload dropped the rigs: they go up once, over the rest poses that just went up, and take their pose
      mRigsResident = false;
      if (rigs) {
        std::vector<sthip_rig_desc> descs(sd.mRigs.size());
        bool posed = false;
        for (size_t i = 0; i < descs.size(); i++) {
          const Scene::SceneData::Rig& r = sd.mRigs[i];
          descs[i] = sthip_rig_desc{};
          descs[i].first_vertex = r.first_vertex, descs[i].vertex_count = r.vertex_count;
          descs[i].blend_target_count = (uint32_t)r.targets.size(), descs[i].bone_count = r.bone_count;
          for (size_t k = 0; k < r.targets.size(); k++) descs[i].blend_targets[k] = r.targets[k].data();
          descs[i].weights = r.bone_count ? r.weights.data() : nullptr;
          posed = posed || sd.mPoses[i].posed;
        }
        if (sthip_scene_set_rigs(mCtx, descs.data(), (uint32_t)descs.size()) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_set_rigs: ") + sthip_last_error(mCtx));
        mRigsResident = true;
        if (posed && animate(sd) != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_animate: ") + sthip_last_error(mCtx));
      }
    }
    mBound = scene->data().get();
    mBoundData = scene->data();
    mPushConstants.gLightCount = d.light_count;                    // BDPT.cpp:396
    mPushConstants.gEnvironmentMaterialAddress = scene->data()->mEnvironmentMaterialAddress;  // BDPT.cpp:393
  }

  // what a frame hands to sthip_render: the view arrays, the push constants and the scene flags as BDPT::render resolves
  // them (BDPT.cpp:444-503). Shared by the single-device render below and the multi-device one (stratum_hip_multi.hpp).
  struct FrameSetup {
    std::vector<ViewData> v;
    std::vector<TransformData> t, ti;
    std::vector<uint32_t> view_media;
    sthip_frame_desc f{};
    BDPTPushConstants pc{};
    uint32_t scene_flags = 0;
  };
  void prepare_frame(uint32_t width, uint32_t height, const std::vector<std::pair<ViewData, TransformData>>& views, FrameSetup& fs) const {
    if (!mBound) throw std::runtime_error("BDPT::render: no scene bound (Scene::update / BDPT::update have not run)");
    std::vector<ViewData>& v = fs.v;
    std::vector<TransformData>&t = fs.t, &ti = fs.ti;
    for (const auto& p : views) {
      v.push_back(p.first);
      t.push_back(p.second);
      ti.push_back(inverse(p.second));  // BDPT.cpp:448-452
    }
    sthip_frame_desc& f = fs.f;
    f.gViews = v.data();
    f.gViewTransforms = t.data();
    f.gInverseViewTransforms = ti.data();
    f.gPrevViews = mPrevViews.size() == v.size() ? mPrevViews.data() : nullptr;
    f.gPrevInverseViewTransforms = mPrevInverseViewTransforms.size() == ti.size() ? mPrevInverseViewTransforms.data() : nullptr;
    f.view_count = (uint32_t)views.size();
    BDPTPushConstants& pc = fs.pc;
    pc = mPushConstants;
    pc.gOutputExtent[0] = width;
    pc.gOutputExtent[1] = height;
    pc.gViewCount = f.view_count;
    if (!((mSamplingFlags >> STHIP_eLVC) & 1u)) pc.gLightPathCount = width * height;  // BDPT.cpp:469-470: with the cache on it stays the user's value
    uint32_t& scene_flags = fs.scene_flags;  // BDPT.cpp:486-503
    scene_flags = 0;
    if (pc.gEnvironmentMaterialAddress != ~0u)
      scene_flags |= STHIP_BDPT_FLAG_HAS_ENVIRONMENT;
    else
      pc.gEnvironmentSampleProbability = 0;
    if (pc.gLightCount)
      scene_flags |= STHIP_BDPT_FLAG_HAS_EMISSIVES;
    else
      pc.gEnvironmentSampleProbability = 1;
    // media: BDPT.cpp:456-466 (the volume instance each camera is inside of) and :497-500
    std::vector<uint32_t>& view_media = fs.view_media;
    view_media.assign(views.size(), 0xFFFFu);
    if (!mBoundData->mMediumInstances.empty()) {
      scene_flags |= STHIP_BDPT_FLAG_HAS_MEDIA;
      for (const auto& mi : mBoundData->mMediumInstances) {
        double box[6];
        if (!mi.first->world_bbox(box)) continue;
        const TransformData& inv = mBoundData->mInstanceInverseTransforms[mi.second];
        for (size_t i = 0; i < views.size(); i++) {
          const TransformData& vt = views[i].second;
          double p[3];
          for (int a = 0; a < 3; a++) p[a] = (double)inv.m[a][0] * vt.m[0][3] + (double)inv.m[a][1] * vt.m[1][3] + (double)inv.m[a][2] * vt.m[2][3] + inv.m[a][3];
          if (p[0] >= box[0] && p[1] >= box[1] && p[2] >= box[2] && p[0] <= box[3] && p[1] <= box[4] && p[2] <= box[5]) view_media[i] = mi.second;
        }
      }
      f.gViewMediumInstances = view_media.data();
    } else {
      pc.gMaxNullCollisions = 0;
    }
  }

  // BDPT::render (BDPT.cpp:423-838) for the hot path: one sample per pixel per call, seed = frame number (:480)
  virtual void render(CommandBuffer& cb, uint32_t width, uint32_t height, const std::vector<std::pair<ViewData, TransformData>>& views, uint32_t seed_count = 1) {
    FrameSetup fs;
    prepare_frame(width, height, views, fs);
    const sthip_frame_desc& f = fs.f;
    const BDPTPushConstants& pc = fs.pc;
    const uint32_t scene_flags = fs.scene_flags;
    Frame fr;
    fr.width = width;
    fr.height = height;
    const size_t n = (size_t)width * height;
    fr.mPrevUVs.assign(2 * n, 0.f);
    fr.mVisibility.assign(n, VisibilityInfo{});
    fr.mDepth.assign(n, DepthInfo{});
    sthip_outputs o{};
    if (mHalfColorPrecision) {  // the float* of the ABI points at halves
      fr.mRadiance16.assign(4 * n, 0);
      fr.mAlbedo16.assign(4 * n, 0);
      o.gRadiance = reinterpret_cast<float*>(fr.mRadiance16.data());
      o.gAlbedo = reinterpret_cast<float*>(fr.mAlbedo16.data());
    } else {
      fr.mRadiance.assign(4 * n, 0.f);
      fr.mAlbedo.assign(4 * n, 0.f);
      o.gRadiance = fr.mRadiance.data();
      o.gAlbedo = fr.mAlbedo.data();
    }
    o.gVisibility = fr.mVisibility.data();
    o.gDepth = fr.mDepth.data();
    o.gPrevUVs = fr.mPrevUVs.data();
    o.gRayCount = fr.mRayCount;
    if (mDebugMode != STHIP_DEBUG_NONE) {  // BDPT.cpp:526-541 (gDebugMode), :560: the image persists from frame to frame
      o.debug_mode = mDebugMode;
      if (mHalfColorPrecision) {
        if (mDebugImage16.size() != 4 * n) mDebugImage16.assign(4 * n, 0);
        o.gDebugImage = reinterpret_cast<float*>(mDebugImage16.data());
      } else {
        if (mDebugImage.size() != 4 * n) mDebugImage.assign(4 * n, 0.f);
        o.gDebugImage = mDebugImage.data();
      }
    }
    (void)sthip_set_stream(mCtx, cb.hip_stream);
    // BDPT.cpp:474,482-483: a frame whose first camera moved since the last one reuses nothing (gReservoirSpatialM = 0) unless the
    // denoiser reprojects; setting the option drops the grids the last frame left (include/sthip.h)
    const bool changed = !mPrevInverseViewTransforms.empty() && !fs.ti.empty() && std::memcmp(&mPrevInverseViewTransforms[0], &fs.ti[0], sizeof(TransformData)) != 0;
    if (auto denoiser = mNode.find<Denoiser>()) mReprojection = denoiser->reprojection();  // BDPT.cpp:472-473
    if (changed && !mReprojection) (void)sthip_set_option(mCtx, "reuse_grids_persist", 1);
    mChanged = changed;
    if (sthip_render(mCtx, &pc, mSamplingFlags, scene_flags, &f, mFrameNumber, seed_count, &o) != STHIP_OK)
      throw std::runtime_error(std::string("sthip_render: ") + sthip_last_error(mCtx));
    if (mDebugMode != STHIP_DEBUG_NONE) {
      if (mHalfColorPrecision)
        fr.mDebugImage16 = mDebugImage16;
      else
        fr.mDebugImage = mDebugImage;
    }
    finish_frame(std::move(fr), fs, seed_count);
  }
  // render() in two halves, for a host that keeps frames in flight (include/sthip.h: sthip_render_async): submit() enqueues the
  // frame — the path on `cb`'s stream, the read-back on the library's copy stream into a set of PINNED buffers this object owns
  // — and returns a ticket; finish(ticket) waits for that frame's outputs, runs the tone map block and makes the frame
  // prev_result(), as render() does. Frames are finished in the order they were submitted. Frame i + 1 renders while frame i
  // copies back as long as no more than "output_ring" (2) frames are submitted and not yet in host memory. The frame number and
  // the "previous views" advance at submit (note_submitted). Not with a debug mode (the debug image chains through host memory).
  // finish() copies the pinned images into the Frame's vectors (prev_result() keeps its type); a host that wants the pinned
  // bytes themselves reads them through the ABI. Non-virtual, and the only code that refers to the pipelined entry points.
  uint64_t submit(CommandBuffer& cb, uint32_t width, uint32_t height, const std::vector<std::pair<ViewData, TransformData>>& views, uint32_t seed_count = 1) {
    if (mDebugMode != STHIP_DEBUG_NONE) throw std::runtime_error("BDPT::submit: not with a debug mode: use render()");
    if (mDenoise && mNode.find<Denoiser>()) throw std::runtime_error("BDPT::submit: not with a Denoiser in the graph (its history chains through host memory): use render()");
    FrameSetup fs;
    prepare_frame(width, height, views, fs);
    if (!mAsync) {
      mAsync = std::shared_ptr<AsyncRing>(new AsyncRing{mCtx, {}}, [](AsyncRing* r) {
        for (AsyncSet& a : r->sets) (void)sthip_host_free(r->ctx, a.block);
        delete r;
      });
    }
    const size_t n = (size_t)width * height, cb_bytes = mHalfColorPrecision ? 8 : 16;
    const size_t bytes = n * (2 * cb_bytes + 8 + 16 + 8) + 16;
    AsyncSet* set = nullptr;
    for (AsyncSet& a : mAsync->sets)
      if (a.ticket == 0) set = &a;
    if (!set) {
      mAsync->sets.push_back(AsyncSet{});
      set = &mAsync->sets.back();
    }
    if (set->bytes != bytes) {
      if (set->block && sthip_host_free(mCtx, set->block) != STHIP_OK) throw std::runtime_error(std::string("sthip_host_free: ") + sthip_last_error(mCtx));
      set->block = nullptr;
      set->bytes = 0;
      if (sthip_host_alloc(mCtx, bytes, &set->block) != STHIP_OK) throw std::runtime_error(std::string("sthip_host_alloc: ") + sthip_last_error(mCtx));
      set->bytes = bytes;
    }
    set->width = width;
    set->height = height;
    set->half = mHalfColorPrecision;
    uint8_t* q = static_cast<uint8_t*>(set->block);
    sthip_outputs o{};
    o.gRadiance = reinterpret_cast<float*>(q);
    o.gAlbedo = reinterpret_cast<float*>(q + n * cb_bytes);
    o.gVisibility = reinterpret_cast<VisibilityInfo*>(q + 2 * n * cb_bytes);
    o.gDepth = reinterpret_cast<DepthInfo*>(q + 2 * n * cb_bytes + 8 * n);
    o.gPrevUVs = reinterpret_cast<float*>(q + 2 * n * cb_bytes + 24 * n);
    o.gRayCount = reinterpret_cast<uint64_t*>(q + 2 * n * cb_bytes + 32 * n);
    (void)sthip_set_stream(mCtx, cb.hip_stream);
    const bool changed = !mPrevInverseViewTransforms.empty() && !fs.ti.empty() && std::memcmp(&mPrevInverseViewTransforms[0], &fs.ti[0], sizeof(TransformData)) != 0;
    if (changed && !mReprojection) (void)sthip_set_option(mCtx, "reuse_grids_persist", 1);  // (as render())
    uint64_t ticket = 0;
    if (sthip_render_async(mCtx, &fs.pc, mSamplingFlags, fs.scene_flags, &fs.f, mFrameNumber, seed_count, &o, &ticket) != STHIP_OK)
      throw std::runtime_error(std::string("sthip_render_async: ") + sthip_last_error(mCtx));
    set->ticket = ticket;
    note_submitted(fs, seed_count);
    return ticket;
  }
  void finish(uint64_t ticket) {
    AsyncSet* set = nullptr;
    if (mAsync)
      for (AsyncSet& a : mAsync->sets)
        if (a.ticket == ticket && ticket != 0) set = &a;
    if (!set) throw std::runtime_error("BDPT::finish: no such frame in flight");
    if (sthip_wait_outputs(mCtx, ticket) != STHIP_OK) throw std::runtime_error(std::string("sthip_wait_outputs: ") + sthip_last_error(mCtx));
    Frame fr;
    fr.width = set->width;
    fr.height = set->height;
    const size_t n = (size_t)set->width * set->height, cb_bytes = set->half ? 8 : 16;
    const uint8_t* q = static_cast<const uint8_t*>(set->block);
    if (set->half) {
      fr.mRadiance16.assign(reinterpret_cast<const uint16_t*>(q), reinterpret_cast<const uint16_t*>(q) + 4 * n);
      fr.mAlbedo16.assign(reinterpret_cast<const uint16_t*>(q + n * cb_bytes), reinterpret_cast<const uint16_t*>(q + n * cb_bytes) + 4 * n);
    } else {
      fr.mRadiance.assign(reinterpret_cast<const float*>(q), reinterpret_cast<const float*>(q) + 4 * n);
      fr.mAlbedo.assign(reinterpret_cast<const float*>(q + n * cb_bytes), reinterpret_cast<const float*>(q + n * cb_bytes) + 4 * n);
    }
    const uint8_t* g = q + 2 * n * cb_bytes;
    fr.mVisibility.assign(reinterpret_cast<const VisibilityInfo*>(g), reinterpret_cast<const VisibilityInfo*>(g) + n);
    fr.mDepth.assign(reinterpret_cast<const DepthInfo*>(g + 8 * n), reinterpret_cast<const DepthInfo*>(g + 8 * n) + n);
    fr.mPrevUVs.assign(reinterpret_cast<const float*>(g + 24 * n), reinterpret_cast<const float*>(g + 24 * n) + 2 * n);
    std::memcpy(fr.mRayCount, g + 32 * n, 16);
    set->ticket = 0;
    finish_frame(std::move(fr), FrameSetup{}, 0, true);
  }

  // BDPTDebugMode (bdpt.h:177-193; the inspector's "Debug mode", BDPT.cpp:253-262) with mPushConstants.gDebugViewPathLength /
  // gDebugLightPathLength; the image starts from zero when the mode or the frame size changes
  void set_debug_mode(uint32_t mode) {
    if (mode != mDebugMode) {
      mDebugImage.clear();
      mDebugImage16.clear();
    }
    mDebugMode = mode < STHIP_DEBUG_MODE_COUNT ? mode : (uint32_t)STHIP_DEBUG_NONE;
  }
  uint32_t debug_mode() const { return mDebugMode; }
  // Denoiser::reprojection() (BDPT.cpp:472-473): with it a moving camera keeps the previous frame's reuse grids
  // (with a Denoiser in the graph render() takes it from the component instead)
  void set_reprojection(bool on) { mReprojection = on; }
  bool& denoise() { return mDenoise; }  // "Enable denoiser" (BDPT.cpp:302): whether a Denoiser in the graph is used

 protected:
  uint32_t frame_number() const { return mFrameNumber; }
  uint32_t sampling_flags() const { return mSamplingFlags; }
  // the bookkeeping of a frame that has been handed to the device(s): the next frame's seed and its "previous views"
  // (BDPT.cpp:480,563). finish_frame does it itself unless told that the frame was noted when it was submitted (frames in flight).
  void note_submitted(const FrameSetup& fs, uint32_t seed_count) {
    mFrameNumber += seed_count;
    mPrevViews = fs.v;
    mPrevInverseViewTransforms = fs.ti;
  }
  // what follows the path in BDPT::render: the tone map block and the frame bookkeeping
  void finish_frame(Frame fr, const FrameSetup& fs, uint32_t seed_count, bool noted_at_submit = false) {
    const uint32_t width = fr.width, height = fr.height;
    const size_t n = (size_t)width * height;
    // tone map (BDPT.cpp:783-815); without a Denoiser in the graph gModulateAlbedo stays off (:779-780 only run when one exists)
    sthip_tonemap_desc tm{};
    if (mHalfColorPrecision) {  // (the context's option makes all three images RGBA16F)
      if (fr.mAlbedo16.size() != 4 * n) fr.mAlbedo16.assign(4 * n, 0);
      fr.mTonemapResult16.assign(4 * n, 0);
      tm.gInput = reinterpret_cast<const float*>(fr.mDebugImage16.size() == 4 * n ? fr.mDebugImage16.data() : fr.mRadiance16.data());
      tm.gAlbedo = reinterpret_cast<const float*>(fr.mAlbedo16.data());
      tm.gOutput = reinterpret_cast<float*>(fr.mTonemapResult16.data());
    } else {
      if (fr.mAlbedo.size() != 4 * n) fr.mAlbedo.assign(4 * n, 0.f);
      fr.mTonemapResult.assign(4 * n, 0.f);
      tm.gInput = fr.mDebugImage.size() == 4 * n ? fr.mDebugImage.data() : fr.mRadiance.data();  // BDPT.cpp:764: with a debug mode the debug image is what is shown
      tm.gAlbedo = fr.mAlbedo.data();
      tm.gOutput = fr.mTonemapResult.data();
    }
    tm.width = width;
    tm.height = height;
    tm.mode = mTonemapMode;
    tm.modulate_albedo = 0;
    if (auto denoiser = mDenoise ? mNode.find<Denoiser>() : component_ptr<Denoiser>()) {  // accumulate / denoise, BDPT.cpp:767-781
      if (mChanged && !denoiser->reprojection()) denoiser->reset_accumulation();
      const void* albedo = mHalfColorPrecision ? static_cast<const void*>(fr.mAlbedo16.data()) : static_cast<const void*>(fr.mAlbedo.data());
      const void* result = denoiser->denoise(mCtx, mHalfColorPrecision, width, height, tm.gInput, albedo, fs.v, fr.mVisibility, fr.mDepth, fr.mPrevUVs);
      if (mHalfColorPrecision)
        fr.mDenoiseResult16.assign(static_cast<const uint16_t*>(result), static_cast<const uint16_t*>(result) + 4 * n);
      else
        fr.mDenoiseResult.assign(static_cast<const float*>(result), static_cast<const float*>(result) + 4 * n);
      tm.gInput = mHalfColorPrecision ? reinterpret_cast<const float*>(fr.mDenoiseResult16.data()) : fr.mDenoiseResult.data();
      tm.modulate_albedo = denoiser->demodulate_albedo() ? 1u : 0u;
    }
    tm.gamma_correction = mGammaCorrection ? 1u : 0u;
    tm.exposure = mExposure;
    tm.exposure_alpha = mExposureAlpha;       // gExposureAlpha, BDPT.cpp:51,192,307
    tm.exposure_state = mTonemapState;        // mPrevFrame->mTonemapMax bytes 16..39 -> gPrevMax, BDPT.cpp:810-811
    tm.out_max = fr.mTonemapMax;
    if (sthip_tonemap(mCtx, &tm) != STHIP_OK) throw std::runtime_error(std::string("sthip_tonemap: ") + sthip_last_error(mCtx));
    if (!noted_at_submit) note_submitted(fs, seed_count);
    mPrevFrame = std::move(fr);
  }

 public:
  void reset_frame_number(uint32_t n = 0) { mFrameNumber = n; }

 protected:
  Node& mNode;
  sthip_ctx* mCtx = nullptr;
  const void* mBound = nullptr;
  std::shared_ptr<Scene::SceneData> mBoundData;
  bool mLastUpdateWasTransformsOnly = false, mLastUpdateWasVerticesOnly = false, mLastUpdateWasEnvironmentOnly = false, mLastUpdateWasMaterialsOnly = false;
  bool mVerticesBehindDevice = false;  // set_vertices_device wrote the resident vertices: the bound data's are older
  // false: a changed material is uploaded like any other change. The multi-device driver clears it, as mRefitDeformedMeshes.
  bool mMaterialsOnDevice = true;
  bool mVolumesOnDevice = true;  // MultiDeviceBDPT: false (a changed grid is a full upload on every rank)
  bool mLastUpdateWasVolumesOnly = false;
  uint32_t mVolumeCalls = 0;
  // false: a deformed mesh is uploaded like any other change. The multi-device driver clears it: its ranks must all walk the
  // same tree form, and it sends them uploads or transforms-only updates, nothing else (stratum_hip_multi.hpp).
  bool mRefitDeformedMeshes = true;
  template <typename T>
  static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
  }
  bool mRigsResident = false;  // the rigs of mBoundData are on the device (sthip_scene_set_rigs after the last upload)
  uint32_t mUploadCalls = 0, mEnvironmentCalls = 0, mMaterialDataCalls = 0, mImageCalls = 0;
  // Everything of `b` is what `a` is except bytes of gMaterialData outside the environment record and / or the texels of
  // images (the same objects at the same extents and formats, another serial). An image that is also the environment's keeps
  // the upload: its tables would have to follow.
  static bool materials_only_changed(const Scene::SceneData& a, const Scene::SceneData& b) {
    if (a.mMaterialData.size() != b.mMaterialData.size() || a.mImageSerials.size() != b.mImageSerials.size() || a.mImage1Serials.size() != b.mImage1Serials.size()) return false;
    if (a.mResources.image4s != b.mResources.image4s || a.mResources.image1s != b.mResources.image1s || a.mResources.volumes != b.mResources.volumes) return false;  // the same objects
    bool changed = !same_bytes(a.mMaterialData, b.mMaterialData);
    for (size_t i = 0; i < b.mImageSerials.size(); i++) {
      if (a.mImageDescs[i].width != b.mImageDescs[i].width || a.mImageDescs[i].height != b.mImageDescs[i].height || a.mImageFormats[i] != b.mImageFormats[i]) return false;
      if (a.mImageSerials[i] == b.mImageSerials[i]) continue;
      if (b.mResources.image4s[i] == b.mEnvironmentImage) return false;
      changed = true;
    }
    for (size_t i = 0; i < b.mImage1Serials.size(); i++) {
      if (a.mImage1Descs[i].width != b.mImage1Descs[i].width || a.mImage1Descs[i].height != b.mImage1Descs[i].height || a.mImage1Formats[i] != b.mImage1Formats[i]) return false;
      changed = changed || a.mImage1Serials[i] != b.mImage1Serials[i];
    }
    if (!changed) return false;
    if (a.mEnvironmentMaterialAddress != b.mEnvironmentMaterialAddress || a.mEnvironmentImage != b.mEnvironmentImage || a.mEnvironmentImageSerial != b.mEnvironmentImageSerial ||
        a.mEnvironmentTablesOnDevice != b.mEnvironmentTablesOnDevice)
      return false;
    return same_rigs(a, b) && same_poses(a, b) && same_bytes(a.mVertices, b.mVertices) && same_bytes(a.mIndices, b.mIndices) && same_bytes(a.mInstances, b.mInstances) &&
           same_bytes(a.mLightInstanceMap, b.mLightInstanceMap) && same_bytes(a.mInstanceTransforms, b.mInstanceTransforms) && same_bytes(a.mInstanceInverseTransforms, b.mInstanceInverseTransforms) &&
           same_bytes(a.mInstanceMotionTransforms, b.mInstanceMotionTransforms) && same_bytes(a.mDistributionData, b.mDistributionData);
  }
  // The differing byte range, then the differing images in one call. STHIP_ERR_UNSUPPORTED from the bytes: nothing has changed
  // and the caller uploads.
  int set_materials(const Scene::SceneData& a, const Scene::SceneData& b) {
    size_t lo = 0, hi = b.mMaterialData.size();
    while (lo < hi && a.mMaterialData[lo] == b.mMaterialData[lo]) lo++;
    while (hi > lo && a.mMaterialData[hi - 1] == b.mMaterialData[hi - 1]) hi--;
    if (hi > lo) {
      mMaterialDataCalls++;
      const int rc = sthip_scene_set_material_data(mCtx, (uint32_t)(lo * 4), &b.mMaterialData[lo], (uint32_t)((hi - lo) * 4), nullptr);
      if (rc == STHIP_ERR_UNSUPPORTED) return rc;
      if (rc != STHIP_OK) throw std::runtime_error(std::string("sthip_scene_set_material_data: ") + sthip_last_error(mCtx));
    }
    std::vector<sthip_image_update> entries;
    for (size_t i = 0; i < b.mImageSerials.size(); i++)
      if (a.mImageSerials[i] != b.mImageSerials[i]) entries.push_back(sthip_image_update{0u, (uint32_t)i, b.mImageDescs[i].pixels, b.mImageDescs[i].width, b.mImageDescs[i].height, 0u, 0u});
    for (size_t i = 0; i < b.mImage1Serials.size(); i++)
      if (a.mImage1Serials[i] != b.mImage1Serials[i]) entries.push_back(sthip_image_update{1u, (uint32_t)i, b.mImage1Descs[i].pixels, b.mImage1Descs[i].width, b.mImage1Descs[i].height, 0u, 0u});
    if (!entries.empty()) {
      mImageCalls++;
      if (sthip_scene_set_images(mCtx, entries.data(), (uint32_t)entries.size(), (uint32_t)sizeof(sthip_image_update), nullptr) != STHIP_OK)
        throw std::runtime_error(std::string("sthip_scene_set_images: ") + sthip_last_error(mCtx));
    }
    return STHIP_OK;
  }
  // Everything of `b` is what `a` is except the value of the environment record, the texels of its image (the same object,
  // another serial) and the tables that follow from them: the comparison same_poses is for the rigs.
  static bool environment_only_changed(const Scene::SceneData& a, const Scene::SceneData& b) {
    const uint32_t addr = b.mEnvironmentMaterialAddress;
    if (addr == ~0u || a.mEnvironmentMaterialAddress != addr || a.mEnvironmentImage != b.mEnvironmentImage) return false;
    if (a.mMaterialData.size() != b.mMaterialData.size() || (size_t)addr / 4 + 4 > b.mMaterialData.size()) return false;
    const size_t at = addr / 4;
    const bool value_changed = std::memcmp(&a.mMaterialData[at], &b.mMaterialData[at], 12) != 0;
    const bool image_changed = b.mEnvironmentImage && a.mEnvironmentImageSerial != b.mEnvironmentImageSerial;
    if (!value_changed && !image_changed) return false;
    if (image_changed && !b.mEnvironmentImage->bytes.empty()) return false;  // (an 8-bit environment: nothing the call serves)
    if (std::memcmp(a.mMaterialData.data(), b.mMaterialData.data(), at * 4) || std::memcmp(&a.mMaterialData[at + 3], &b.mMaterialData[at + 3], (b.mMaterialData.size() - at - 3) * 4)) return false;
    if (!image_changed && !same_bytes(a.mDistributionData, b.mDistributionData)) return false;
    if (a.mDistributionData.size() != b.mDistributionData.size()) return false;
    if (!same_rigs(a, b) || !same_poses(a, b) || !same_bytes(a.mVertices, b.mVertices) || !same_bytes(a.mIndices, b.mIndices) || !same_bytes(a.mInstances, b.mInstances) ||
        !same_bytes(a.mLightInstanceMap, b.mLightInstanceMap) || !same_bytes(a.mInstanceTransforms, b.mInstanceTransforms) || !same_bytes(a.mInstanceInverseTransforms, b.mInstanceInverseTransforms) ||
        !same_bytes(a.mInstanceMotionTransforms, b.mInstanceMotionTransforms))
      return false;
    return a.mResources.image4s == b.mResources.image4s && a.mResources.image1s == b.mResources.image1s && a.mResources.volumes == b.mResources.volumes;  // the same objects
  }
  int set_environment(const Scene::SceneData& a, const Scene::SceneData& b) {
    const size_t at = b.mEnvironmentMaterialAddress / 4;
    sthip_environment_desc e{};
    e.struct_size = sizeof(e);
    e.material_address = b.mEnvironmentMaterialAddress;
    if (std::memcmp(&a.mMaterialData[at], &b.mMaterialData[at], 12)) e.value = reinterpret_cast<const float*>(&b.mMaterialData[at]);
    if (b.mEnvironmentImage && a.mEnvironmentImageSerial != b.mEnvironmentImageSerial) {
      e.pixels = b.mEnvironmentImage->pixels.data();
      e.width = b.mEnvironmentImage->width, e.height = b.mEnvironmentImage->height;
    }
    mEnvironmentCalls++;
    const int rc = sthip_scene_set_environment(mCtx, &e, nullptr);
    if (rc != STHIP_OK && rc != STHIP_ERR_UNSUPPORTED) throw std::runtime_error(std::string("sthip_scene_set_environment: ") + sthip_last_error(mCtx));
    return rc;
  }
  // sthip_scene_animate with the poses of `sd`. The call poses every rig; one whose mesh never got a pose is sent zero factors
  // and identity bones (its positions stay the rest pose's; its normals are normalised again if it has blend targets).
  int animate(const Scene::SceneData& sd) {
    std::vector<sthip_rig_pose> poses(sd.mPoses.size());
    std::vector<std::vector<TransformData>> identity(sd.mPoses.size());
    for (size_t i = 0; i < poses.size(); i++) {
      poses[i] = sthip_rig_pose{};
      std::memcpy(poses[i].blend_factors, sd.mPoses[i].factors, sizeof(poses[i].blend_factors));
      const uint32_t bone_count = sd.mRigs[i].bone_count;
      if (sd.mPoses[i].bones.size() == bone_count) {
        poses[i].bones = bone_count ? sd.mPoses[i].bones.data() : nullptr;
      } else {  // (never posed: identity bones)
        TransformData I{};
        I.m[0][0] = I.m[1][1] = I.m[2][2] = 1;
        identity[i].assign(bone_count, I);
        poses[i].bones = identity[i].data();
      }
    }
    const int rc = sthip_scene_animate(mCtx, poses.data(), (uint32_t)poses.size(), nullptr);
    if (rc != STHIP_OK && rc != STHIP_ERR_UNSUPPORTED) throw std::runtime_error(std::string("sthip_scene_animate: ") + sthip_last_error(mCtx));
    return rc;
  }
  static bool same_poses(const Scene::SceneData& a, const Scene::SceneData& b) {
    if (a.mPoses.size() != b.mPoses.size()) return false;
    for (size_t i = 0; i < a.mPoses.size(); i++)
      if (a.mPoses[i].posed != b.mPoses[i].posed || std::memcmp(a.mPoses[i].factors, b.mPoses[i].factors, sizeof(a.mPoses[i].factors)) || !same_bytes(a.mPoses[i].bones, b.mPoses[i].bones)) return false;
    return true;
  }
  static bool same_rigs(const Scene::SceneData& a, const Scene::SceneData& b) {
    if (a.mRigs.size() != b.mRigs.size()) return false;
    for (size_t i = 0; i < a.mRigs.size(); i++) {
      const Scene::SceneData::Rig &x = a.mRigs[i], &y = b.mRigs[i];
      if (x.first_vertex != y.first_vertex || x.vertex_count != y.vertex_count || x.bone_count != y.bone_count || x.targets.size() != y.targets.size() || !same_bytes(x.weights, y.weights)) return false;
      for (size_t k = 0; k < x.targets.size(); k++)
        if (!same_bytes(x.targets[k], y.targets[k])) return false;
    }
    return true;
  }
  static bool same_volume_serials(const Scene::SceneData& a, const Scene::SceneData& b) { return a.mVolumeSerials == b.mVolumeSerials; }
  // everything of `b` is what `a` is except the grids behind some of the same volume objects
  static bool volumes_only_changed(const Scene::SceneData& a, const Scene::SceneData& b) {
    return same_geometry(a, b) && same_poses(a, b) && a.mVolumeMedia == b.mVolumeMedia && same_bytes(a.mInstanceTransforms, b.mInstanceTransforms) &&
           same_bytes(a.mInstanceInverseTransforms, b.mInstanceInverseTransforms) && same_bytes(a.mInstanceMotionTransforms, b.mInstanceMotionTransforms);
  }
  // the changed grids into the resident scene; a refusal the library words as unsupported or invalid leaves the upload to the caller
  int set_volumes(const Scene::SceneData& a, const Scene::SceneData& b) {
    for (size_t i = 0; i < b.mVolumeSerials.size(); i++) {
      if (a.mVolumeSerials[i] == b.mVolumeSerials[i]) continue;
      const Medium* m = b.mVolumeMedia[i];
      if (!m) return STHIP_ERR_UNSUPPORTED;
      sthip_volume_source s{};
      s.struct_size = sizeof(s);
      sthip_dense_volume_desc d{};
      if (m->dense_pending) {
        d = m->dense_desc();
        s.dense = &d;
      } else {
        s.data = m->density_buffer->data();
        s.bytes = m->density_buffer->size();
      }
      sthip_volume_info info{};
      mVolumeCalls++;
      const int rc = sthip_scene_set_volume(mCtx, (uint32_t)i, &s, &info);
      if (rc == STHIP_ERR_HIP || rc == STHIP_ERR_NO_SCENE) throw std::runtime_error(std::string("sthip_scene_set_volume: ") + sthip_last_error(mCtx));
      if (rc != STHIP_OK) return rc;
      if (m->dense_pending) {
        m->dense_pending = false;
        m->device_grid_newer = true;
        m->has_device_world_bbox = true;
        std::memcpy(m->device_world_bbox, info.world_bbox, 48);
      }
    }
    return STHIP_OK;
  }
  static bool same_geometry(const Scene::SceneData& a, const Scene::SceneData& b) { return same_bytes(a.mVertices, b.mVertices) && same_topology(a, b); }
  // everything equal except the CONTENTS of the vertex array (and the transforms, which have update calls of their own)
  static bool same_topology(const Scene::SceneData& a, const Scene::SceneData& b) {
    if (!same_rigs(a, b)) return false;
    if (a.mVertices.size() != b.mVertices.size() || !same_bytes(a.mIndices, b.mIndices) || !same_bytes(a.mInstances, b.mInstances) || !same_bytes(a.mMaterialData, b.mMaterialData) ||
        !same_bytes(a.mLightInstanceMap, b.mLightInstanceMap) || !same_bytes(a.mDistributionData, b.mDistributionData))
      return false;
    if (a.mResources.image4s != b.mResources.image4s || a.mResources.image1s != b.mResources.image1s || a.mResources.volumes != b.mResources.volumes) return false;  // the same objects
    if (a.mImageSerials != b.mImageSerials || a.mImage1Serials != b.mImage1Serials) return false;  // ... with the same texels (Image::mark_dirty())
    // (an environment whose tables the device builds packs the same bytes before and after Environment::mark_image_dirty():
    // the image's serial is what tells the texels apart, and a partial update must not pass over a changed sky)
    return a.mEnvironmentMaterialAddress == b.mEnvironmentMaterialAddress && a.mEnvironmentImage == b.mEnvironmentImage && a.mEnvironmentImageSerial == b.mEnvironmentImageSerial &&
           a.mEnvironmentTablesOnDevice == b.mEnvironmentTablesOnDevice;
  }
  uint32_t mSamplingFlags = 0;
  BDPTPushConstants mPushConstants;
  uint32_t mFrameNumber = 0;
  uint32_t mDebugMode = STHIP_DEBUG_NONE;
  bool mReprojection = false;
  bool mDenoise = true;   // BDPT.hpp: mDenoise = true
  bool mChanged = false;  // the frame being rendered moved its first camera (render() -> finish_frame)
  std::vector<float> mDebugImage;
  bool mHalfColorPrecision = false;  // BDPT.cpp:231
  std::vector<uint16_t> mDebugImage16;  // mDebugImage while mHalfColorPrecision is on
  uint32_t mTonemapMode = STHIP_TONEMAP_RAW;  // BDPT.cpp:48
  float mExposure = 0;
  float mExposureAlpha = 0;
  float mTonemapState[6] = {0, 0, 0, 0, 0, 0};
  bool mGammaCorrection = true;
  std::vector<ViewData> mPrevViews;
  std::vector<TransformData> mPrevInverseViewTransforms;
  // submit() / finish(): a set of pinned images per frame in flight (sthip_host_alloc), owned through a handle whose deleter
  // submit() installs — nothing else here refers to the pipelined entry points
  struct AsyncSet {
    void* block = nullptr;  // radiance | albedo | visibility | depth | prev-uv | gRayCount
    size_t bytes = 0;
    uint64_t ticket = 0;  // 0: free
    uint32_t width = 0, height = 0;
    bool half = false;
  };
  struct AsyncRing {
    sthip_ctx* ctx;
    std::vector<AsyncSet> sets;
  };
  std::shared_ptr<AsyncRing> mAsync;
  Frame mPrevFrame;
};

// ---------------------------------------------------------------------------------------------
// Plugin loading: the component main.cpp attaches per `--plugin=<lib>;<fn>;<fn>...` argument
// (src/main.cpp:11-24,148-149) over src/Common/dynamic_library.hpp:7-59. Same contract: the library is opened
// with RTLD_NOW when the component is made and stays loaded for the component's life; invoke<R, Args...>(name, args...)
// resolves `name` once (cached) and calls it as R(*)(Args...); a library that does not load throws runtime_error, a
// missing symbol invalid_argument.
// ---------------------------------------------------------------------------------------------
class dynamic_library {
 public:
  // RTLD_NODELETE: components a plugin function makes carry deleters whose code lives in the plugin, and a node graph
  // destroys its components in no particular order — dlclose() then only drops the handle, the code stays mapped
  explicit dynamic_library(const std::string& filename) : mHandle(dlopen(filename.c_str(), RTLD_NOW | RTLD_NODELETE)) {
    if (!mHandle) {
      const char* why = dlerror();
      throw std::runtime_error("Failed to load " + filename + (why ? std::string(": ") + why : std::string()));
    }
  }
  dynamic_library(const dynamic_library&) = delete;
  dynamic_library& operator=(const dynamic_library&) = delete;
  ~dynamic_library() {
    if (mHandle) dlclose(mHandle);
  }
  template <typename return_t, typename... Args>
  return_t invoke(const std::string& name, Args... args) {
    auto it = mFunctionPtrs.find(name);
    if (it == mFunctionPtrs.end()) it = mFunctionPtrs.emplace(name, dlsym(mHandle, name.c_str())).first;
    if (!it->second) throw std::invalid_argument("Could not find function " + name);
    using fn_t = return_t (*)(Args...);
    return reinterpret_cast<fn_t>(it->second)(std::forward<Args>(args)...);
  }

 private:
  void* mHandle;
  std::unordered_map<std::string, void*> mFunctionPtrs;
};

// `plugin_info` = "<library>;<function>;<function>...": a child node named after the library's stem under `dst` carries the
// dynamic_library component, and every named function is called with that child node (main.cpp:11-24)
inline void load_plugins(const std::string& plugin_info, Node& dst) {
  const size_t first = plugin_info.find(';');
  const std::string filename = plugin_info.substr(0, first);
  std::string stem = filename.substr(filename.find_last_of('/') == std::string::npos ? 0 : filename.find_last_of('/') + 1);
  if (stem.find_last_of('.') != std::string::npos && stem.find_last_of('.') > 0) stem = stem.substr(0, stem.find_last_of('.'));
  auto plugin = dst.make_child(stem).make_component<dynamic_library>(filename);
  for (size_t at = first; at != std::string::npos;) {
    const size_t next = plugin_info.find(';', at + 1);
    const std::string fn = plugin_info.substr(at + 1, next == std::string::npos ? std::string::npos : next - at - 1);
    plugin->invoke<void, Node&>(fn, plugin.node());
    at = next;
  }
}

}  // namespace stm
