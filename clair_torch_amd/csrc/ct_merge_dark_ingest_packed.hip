// ct_merge_dark_ingest_packed.hip -- the interleaved (PACKED3) instantiations of the fused chain + dark-field blur + merge
// kernel, behind ct::merge_dark_ingest_packed (ct_hdr_merge_dark_ingest_batches on CT_LAYOUT_NHWC / NHWC_BGR frames).  The body
// is ct::merge_dark_ingest_kernel of ct_merge_dark_ingest_kernel.hpp; the head of ct_merge_dark_ingest.hip describes the walk
// and its resources.  A translation unit of its own, as ct_merge_dark_multi.hip is for the several-batches kernel: the
// instantiations compile next to the planar ones instead of after them.
#include "ct_merge_dark_ingest_kernel.hpp"

namespace ct {

int merge_dark_ingest_packed(const MergeDarkIngestArgs &a, const MergeDarkIngestBatches &mb, int dtype, int interp, int weight_mode,
                             bool has_std, hipStream_t s)
{
    return mdi_dispatch<true>(a, mb, dtype, interp, weight_mode, has_std, s);
}

}  // namespace ct
