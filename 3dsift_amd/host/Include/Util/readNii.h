// readNii.h -- NIfTI loader with the reference's signature (Include/Util/readNii.h:6).
#pragma once
#include "common.h"

// Reads a NIfTI-1 / NIfTI-2 volume -- single file (.nii) or .hdr + .img pair named by either file, ANALYZE 7.5 pairs, each optionally
// gzip-compressed -- and returns it as a new float[] (caller
// delete[]s), converting the stored datatype to fp32 WITHOUT applying scl_slope / scl_inter, like
// the reference (Src/Util/readNii.cpp:17-33).  Returns nullptr on failure.
SIFT_LIBRARY_API float *readNiiFile(const char *filename, int &nx, int &ny, int &nz);

// Extension (no reference counterpart): the same files with the 8 / 16-bit integer datatypes left as they are stored, for
// CSIFT3DFactory::CreateCSIFT3DTyped and CPUSIFT::UploadVolume, which widen them on the GPU.  NIfTI / ANALYZE datatype 2 (uint8),
// 256 (int8), 4 (int16) and 512 (uint16) come back as the file's own integers -- byte-swapped here where the file is of the other
// byte order -- with type U8 / I8 / I16 / U16; every other datatype comes back as readNiiFile returns it, with type F32.  The same
// headers are accepted and refused.  The caller frees the result with delete[] of the MATCHING element type:
//   F32 delete[] (float *)p, U8 delete[] (uint8_t *)p, I8 delete[] (int8_t *)p, U16 delete[] (uint16_t *)p, I16 delete[] (int16_t *)p.
// Returns nullptr on failure.
SIFT_LIBRARY_API void *readNiiFileTyped(const char *filename, int &nx, int &ny, int &nz, VoxelType &type);
