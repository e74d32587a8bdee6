// The bf16 storage type that kernel templates and launchers are instantiated with.  Plain C++ (no HIP), so that both
// vec16.hpp (device) and dispatch.hpp (host) see the one definition.
#pragma once

namespace dalm {
namespace {

struct bf16_t { unsigned short v; };

}  // namespace
}  // namespace dalm
