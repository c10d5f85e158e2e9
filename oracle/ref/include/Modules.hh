// Stand-in for the header the reference's top-level make generates from Modules.make.
// Only the batch scorers are wanted (src/Mm/Module.cc registers them under this switch).
#pragma once
#define MODULE_MM_BATCH
