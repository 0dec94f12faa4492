/* TEST INFRASTRUCTURE ONLY — empty stand-in: the reference includes this header and its render path uses
 * nothing from it (see cuda_runtime.h in this directory). */
#pragma once
