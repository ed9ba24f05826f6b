// charsmap_handle.hpp -- what an ovtk_charsmap handle holds (api_charsmap.cpp builds it).  api_sentencepiece.cpp launches the
// handle's kernels on a sentence's way into the lattice, inside its own enqueue sequence.
#pragma once

#include "charsmap_kernels.hpp"
#include "runtime.hpp"

struct ovtk_charsmap {
    int device = 0;
    ovtk::CharsmapDev dev{};
    ovtk::DevBuf units, strings, meta;
    int64_t per_byte = 3;   // output bytes an input byte can become
};
