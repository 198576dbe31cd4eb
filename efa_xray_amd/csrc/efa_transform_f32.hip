// The state transform on rows stored as float32: the kernels of efa_transform.hip instantiated with float as the element type of
// the rows in memory (loads widen, stores round once), in a translation unit of their own so that the two sets of
// kernels compile side by side, and under kernel names of their own (profiles and code-object checks tell them apart by name).
#define EFA_TRANSFORM_F32 1
#define k_transform k_transform_f32
#define k_transform_rtps k_transform_rtps_f32
#define k_transform_wide k_transform_wide_f32
#include "efa_transform.hip"
