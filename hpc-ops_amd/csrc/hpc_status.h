// Error convention of the C-ABI (include/hpc_amd.h): 0 = launched, negative = refused.  No HIP header: host-only headers use it.
#pragma once

#define HPC_OK 0
#define HPC_ERR_UNSUPPORTED (-1)
#define HPC_ERR_INVALID (-2)
#define HPC_ERR_LAUNCH (-3)
#define HPC_ERR_TIMEOUT (-4)
