// dspi_wire.cpp — the wire layout of dspi_process_wire / dspi_wire_encode (dspi_wire.h).
#include "dspi_wire.h"

namespace dspi {

bool wire_any_i2s(const int32_t *stream_image, uint32_t n_streams, const uint8_t *active, const uint32_t *image_i2s) {
    for (uint32_t s = 0; s < n_streams; s++)
        if ((!active || active[s]) && image_i2s[(size_t)stream_image[s]] != 0) return true;
    return false;
}

}  // namespace dspi
