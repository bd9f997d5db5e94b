// sg_haplotypes.h -- reference ingest and haplotype assembly (sg_haplotypes.hip), shared with the host API.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sg {

// one contig of the raw FASTA image: raw FASTA lines of fixed width -> base codes
struct DevContig {
  uint64_t raw_off;    // first base in the raw buffer
  uint64_t code_off;   // first code in the encoded reference
  uint64_t length;     // bases
  uint32_t line_bases, line_width;
  uint64_t first_block;  // exclusive prefix of 16-base blocks over the contigs
};
struct DevPiece { uint64_t dst; uint64_t src; uint32_t len; uint32_t pad; };  // absolute byte offsets; pad bit 0: src is in the literals
struct DevPatch { uint64_t dst; uint32_t base; uint32_t pad; };

void launch_ref_scan(const uint8_t* raw, uint64_t n, uint64_t* list, uint32_t cap, uint32_t* count, uint32_t* flags, hipStream_t s);
void launch_ref_ingest(const uint8_t* raw, uint8_t* codes, const DevContig* contigs, uint32_t n_contigs, uint64_t n_blocks,
                       uint32_t* flags, hipStream_t s);
void launch_hap_copy(uint8_t* chains, const uint8_t* ref_codes, const uint8_t* literals, const DevPiece* pieces, uint64_t n, hipStream_t s);
void launch_hap_patch(uint8_t* chains, const DevPatch* patches, uint64_t n, hipStream_t s);
void launch_encode_bytes(uint8_t* buf, uint64_t n, hipStream_t s);
void launch_pack2(const uint8_t* chains, uint64_t bytes, uint32_t* fwd2, uint32_t* rc2, uint16_t* bad, hipStream_t s);   // bytes % 1024 == 0

}  // namespace sg
