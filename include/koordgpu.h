/*
 * koordgpu.h — C ABI of the MI355X Filter/Score evaluation engine for koord-scheduler.
 *
 * This is the drop-in boundary. The reference scheduler (Go, k8s.io/kubernetes v1.35.6 framework
 * wrapped by koordinator's frameworkext) evaluates one pod against every node per scheduling cycle
 * through the plugin interfaces below; a batch-aware plugin (see INTEGRATION.md for the cgo stub)
 * replaces those per-node calls with calls into this library:
 *
 *   fwktype.PreFilterPlugin.PreFilter   pkg/scheduler/plugins/loadaware/load_aware.go:139
 *       -> kg_pods_upload + kg_eval_verify / kg_eval_select (whole-cycle results, one call per batch)
 *   fwktype.FilterPlugin.Filter         pkg/scheduler/plugins/loadaware/load_aware.go:150
 *                                       pkg/scheduler/plugins/nodenumaresource/plugin.go:363
 *                                       upstream noderesources.Fits (restated, reservation/plugin.go:915-965)
 *       -> bit lookup in kg_verify_out.status (per pod, per node)
 *   fwktype.ScorePlugin.Score           pkg/scheduler/plugins/loadaware/load_aware.go:235
 *                                       pkg/scheduler/plugins/nodenumaresource/scoring.go:67
 *       -> lookup in kg_verify_out.score_* (int64, same values the Go plugins return)
 *   selectHost (upstream schedulePod)   -> kg_eval_select (deterministic tie-break)
 *   fwktype.ReservePlugin.Reserve       pkg/scheduler/plugins/loadaware/load_aware.go:226
 *                                       pkg/scheduler/plugins/nodenumaresource/plugin.go:585
 *       -> kg_assume;  Unreserve (load_aware.go:231) -> kg_forget
 *   one-pod-per-cycle replay            -> kg_replay (device-resident Assume between pods)
 *   node informer / NodeMetric / NRT event handlers
 *       (loadaware/pod_assign_cache.go:365-413,498-603) -> kg_snapshot_update_rows
 *
 * Conventions: plain C types only; every input buffer is caller-owned and read synchronously
 * (nothing is retained after a call returns); every output buffer is caller-allocated host memory.
 * Functions return kg_status and never abort; kg_last_error() gives the message of the last failure
 * on a context. Integer semantics are Go's: int64 two's complement, truncating division.
 */
#ifndef KOORDGPU_H
#define KOORDGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KG_ABI_VERSION 14

/* LoadAware resource vector width: the default vectorizer is {cpu, memory}
 * (pkg/scheduler/plugins/loadaware/helper.go:162-173, sorted by name). */
#define KG_LA_R 2
/* Scalar (extended) resources on the NodeResourcesFit path, e.g. kubernetes.io/batch-cpu,
 * kubernetes.io/batch-memory (config/manager/scheduler-config.yaml:21-31). */
#define KG_NSCALAR 2
/* NUMA zones per node supported on device (nodenumaresource/node_allocation.go:221-243). */
#define KG_MAX_ZONES 4
/* DeviceShare: GPU minors per node and per-minor resources {gpu-core, gpu-memory-ratio, gpu-memory}
 * (deviceshare/device_cache.go nodeDevice.deviceTotal / deviceFree, apis/extension/device_share.go). */
#define KG_DEV_MINORS 8
#define KG_DEV_R 3
#define KG_DEV_CORE 0
#define KG_DEV_RATIO 1
#define KG_DEV_MEM 2
/* ElasticQuota resource dimensions {cpu, memory, scalar0, scalar1}: the pod request columns
 * req_cpu, req_mem, sc_req[0], sc_req[1] (elasticquota/plugin.go:279-281). */
#define KG_QUOTA_R 4
/* Reservation resource dimensions {cpu, memory, ephemeral-storage, scalar0, scalar1}
 * (framework.Resource fields used by reservation/plugin.go:915-965). */
#define KG_RSV_R 5

typedef enum kg_status {
    KG_OK = 0,
    KG_INVALID_ARG = 1,
    KG_DEVICE_ERROR = 2,
    KG_OOM = 3,
    KG_UNSUPPORTED = 4, /* feature not on the device path: caller runs the reference plugin */
    KG_NO_DEVICE = 5,
    KG_RESERVE_FAILED = 6, /* kg_assume / kg_assume_ext: the pod's Reserve failed (a BestEffort NUMA allocation,
                            * nodenumaresource/plugin.go:612-623): nothing was applied, the pod stays unscheduled */
} kg_status;

/* Enabled plugins (kg_config.plugins). */
#define KG_PLUGIN_NRF 0x1u  /* upstream NodeResourcesFit: Fits + LeastAllocated score          */
#define KG_PLUGIN_LA 0x2u   /* LoadAwareScheduling (loadaware/load_aware.go)                     */
#define KG_PLUGIN_NUMA 0x4u /* NodeNUMAResource (nodenumaresource/plugin.go, scoring.go)         */
#define KG_PLUGIN_DEV 0x8u  /* DeviceShare GPU fit + score (deviceshare/plugin.go, scoring.go)      */
#define KG_PLUGIN_RSV 0x10u /* Reservation restore / filter / score (reservation/plugin.go, scoring.go) */
#define KG_PLUGIN_QUOTA 0x20u /* ElasticQuota PreFilter gate + Reserve (elasticquota/plugin.go)     */
#define KG_PLUGIN_EXT (KG_PLUGIN_DEV | KG_PLUGIN_RSV | KG_PLUGIN_QUOTA)

/* Node LoadAware flags (kg_node_columns.la_flags). Computed by the host at a frozen snapshot time. */
#define KG_LA_HAS_METRIC 0x1u /* podAssignCache holds a NodeMetric for the node (pod_assign_cache.go:169-172) */
#define KG_LA_NM_NIL 0x2u     /* NodeMetric.Status.NodeMetric == nil (load_aware.go:207-210)               */
#define KG_LA_EXPIRED 0x4u    /* isNodeMetricExpired (helper.go:35-40); set only when NodeMetricExpirationSeconds != nil */
#define KG_LA_PROD_THR 0x8u   /* node filter profile has non-empty ProdUsageThresholds (load_aware.go:162)  */
#define KG_LA_AGG_THR 0x10u   /* node filter profile has an AggregatedUsage profile (load_aware.go:167)     */

/* NUMA topology policies (apis/extension/numa_aware.go:168-171). */
#define KG_NUMA_NONE 0u
#define KG_NUMA_BEST_EFFORT 1u
#define KG_NUMA_RESTRICTED 2u
#define KG_NUMA_SINGLE_NODE 3u

/* Pod flags (kg_pod_columns.flags). */
#define KG_POD_DAEMONSET 0x1u /* owned by a DaemonSet (loadaware/helper.go:141-149)                    */
#define KG_POD_PROD 0x2u      /* GetPodPriorityClassWithDefault == prod (apis/extension/priority_utils.go:37-57) */
#define KG_POD_NUMA_SKIP 0x4u /* PodRequests all zero -> NodeNUMAResource Skip (nodenumaresource/plugin.go:277-283) */
#define KG_POD_HAS_CPU 0x8u   /* "cpu" key present in PodRequests                                       */
#define KG_POD_HAS_MEM 0x10u  /* "memory" key present in PodRequests                                    */
#define KG_POD_CPU_BIND 0x20u /* state.requestCPUBind: LSE/LSR pod with a Full/Spread cpuset bind policy */
#define KG_POD_NON_PREEMPTIBLE 0x40u /* extension.IsPodNonPreemptible (elasticquota/plugin.go:288)     */
/* cpuset binding request of a KG_POD_CPU_BIND pod (plugin.go:319-349: requestCPUBind, the resolved
 * preferred/required CPUBindPolicy, the preferred CPUExclusivePolicy); numCPUsNeeded = req_cpu / 1000. */
#define KG_POD_CPU_POLICY_SHIFT 8    /* 2 bits KG_CPU_BIND_*: cpuBindPolicy (required one if set)        */
#define KG_POD_CPU_REQUIRED 0x400u   /* the policy is RequiredCPUBindPolicy                              */
#define KG_POD_CPU_EXCL_SHIFT 11     /* 2 bits KG_CPU_EXCL_*                                             */
#define KG_POD_RSV_REQUIRED 0x80u    /* pod has a reservation affinity (reservation/transformer.go:148,
                                      * stateData.hasAffinity): must allocate from a reservation      */

/* GPURequirements flags (kg_pod_columns.dev_flags). */
#define KG_GPU_POD_SHARED 0x1u      /* gpuShared: per-GPU gpu-core / memory ratio below 100 (devicehandler_gpu.go:53-96) */
#define KG_GPU_POD_HONOR 0x2u       /* GPUPartitionSpec annotation present: honorGPUPartition                    */
#define KG_GPU_POD_RESTRICTED 0x4u  /* GPUPartitionSpec AllocatePolicy Restricted                                */
#define KG_GPU_POD_RING_BW 0x8u     /* GPUPartitionSpec RingBusBandwidth set (kg_pod_columns.dev_ring_bw)          */
#define KG_GPU_POD_SCOPE_SHIFT 4    /* 3 bits: DeviceTopologyScopeLevel of the required scope (0 none, 2 NUMANode,
                                     * 3 PCIe, 4 Device; apis/extension/device_share.go:185-190)               */
#define KG_GPU_POD_TEMPLATE 0x100u  /* enforceGPUSharedResourceTemplate (deviceshare/utils.go:540-547): the
                                     * allocator starts at allocateByTemplate (allocator_gpu.go:135-159), per
                                     * node key kg_pod_columns.dev_tmpl                                        */

/* Reservation allocate policies (apis/scheduling/v1alpha1 ReservationAllocatePolicy). */
#define KG_RSV_DEFAULT 0u
#define KG_RSV_ALIGNED 1u
#define KG_RSV_RESTRICTED 2u

/* Per-(pod,node) filter status bits (kg_verify_out.status). Plugin order follows the framework's
 * filter order: NodeResourcesFit, LoadAwareScheduling, NodeNUMAResource. */
#define KG_ST_NRF_PODS 0x1u   /* "Too many pods"                          */
#define KG_ST_NRF_CPU 0x2u    /* "Insufficient cpu"                       */
#define KG_ST_NRF_MEM 0x4u    /* "Insufficient memory"                    */
#define KG_ST_NRF_EPH 0x8u    /* "Insufficient ephemeral-storage"         */
#define KG_ST_NRF_SC0 0x10u   /* "Insufficient <scalar 0>"                */
#define KG_ST_NRF_SC1 0x20u   /* "Insufficient <scalar 1>"                */
#define KG_ST_NRF_MASK 0x3Fu
#define KG_ST_LA_EXPIRED 0x100u /* ErrReasonNodeMetricExpired                        */
#define KG_ST_LA_CPU 0x200u     /* ErrReasonUsageExceedThreshold, cpu                */
#define KG_ST_LA_MEM 0x400u     /* ErrReasonUsageExceedThreshold, memory             */
#define KG_ST_LA_AGG 0x800u     /* set with LA_CPU/LA_MEM: "aggregated usage" reason */
#define KG_ST_LA_MASK 0x0F00u
/* NodeNUMAResource Reserve failures of a BestEffort node (the Filter does not admit there, plugin.go:446-455;
 * Reserve runs the topology manager, plugin.go:612-623, and the allocation of its best hint,
 * resource_manager.go:300-309). Reported by kg_replay's out_reason and kg_batch_schedule's status. */
#define KG_ST_NUMA_INSUF_CPU 0x1000u  /* "Insufficient NUMA cpu"                              */
#define KG_ST_NUMA_INSUF_MEM 0x2000u  /* "Insufficient NUMA memory"                           */
#define KG_ST_NUMA_INSUF_NODE 0x4000u /* "node(s) Insufficient NUMA Node resources" (no zones)  */
/* The node is outside the pod's candidate node set (kg_pods_set_node_sets): a Filter of the host's that ran before
 * every koord plugin (nodeSelector / affinity, taints, spec.nodeName, PodTopologySpread, a PreFilterResult) and after
 * the ElasticQuota PreFilter gate. Outside every *_MASK. */
#define KG_ST_NODE_EXCLUDED 0x8000u
#define KG_ST_NUMA_AMP_CPU 0x10000u  /* ErrInsufficientAmplifiedCPU                          */
#define KG_ST_NUMA_CONFLICT 0x20000u /* ErrNotMatchNUMATopology (UnschedulableAndUnresolvable) */
#define KG_ST_NUMA_NO_RES 0x40000u   /* "node(s) missing NUMA resources"                      */
#define KG_ST_NUMA_ALIGN 0x80000u    /* ErrNUMAHintCannotAligned                              */
#define KG_ST_NUMA_UNSATISFIED 0x100000u /* ErrUnsatisfiedNUMAResource: a requested resource has no NUMA hint
                                            (frameworkext/topologymanager/policy.go:166-173)     */
#define KG_ST_NUMA_CPU_TOPO 0x200000u /* ErrInvalidCPUTopology (UnschedulableAndUnresolvable)              */
#define KG_ST_NUMA_CPU_BIND 0x400000u /* ErrCPUBindPolicyConflict / ErrSMTAlignmentError / ErrInvalidRequestedCPUs
                                       * (UnschedulableAndUnresolvable, plugin.go:388-418, util.go:131-135) */
#define KG_ST_NUMA_CPUS 0x800000u     /* ErrNotEnoughCPUs: the required bind policy's CPUs do not cover the pod */
#define KG_ST_NUMA_MASK 0xFF7000u
#define KG_ST_DEV_INSUFFICIENT 0x01000000u /* "Insufficient gpu devices" (Unschedulable, device_allocator.go:432) */
#define KG_ST_DEV_NO_DEVICE 0x02000000u    /* no GPU minors on the node's Device (UnschedulableAndUnresolvable,
                                              devicehandler_gpu.go:41-44)                              */
/* DeviceShare reasons are a 4-bit code: bits 24-25 are its low half, bits 6-7 its high half
 * (KG_ST_DEV_CODE). Codes 3.. come from the GPU allocator (deviceshare/allocator_gpu.go:31-41). */
#define KG_ST_DEV_MASK 0x030000C0u
#define KG_ST_DEV_CODE(st) ((((st) >> 24) & 3u) | ((((st) >> 6) & 3u) << 2))
#define KG_ST_DEV_MAKE(code) (((((uint32_t)(code)) & 3u) << 24) | (((((uint32_t)(code)) >> 2) & 3u) << 6))
#define KG_DEV_CODE_INSUFFICIENT 1u      /* "Insufficient gpu devices" (defaultAllocateDevices)                 */
#define KG_DEV_CODE_NO_DEVICE 2u         /* no GPU minors on the node's Device                                  */
#define KG_DEV_CODE_GPU_DEVICES 3u       /* ErrInsufficientGPUDevices: the topology-tree allocation failed       */
#define KG_DEV_CODE_TOPO_SCOPED 4u       /* ErrInsufficientTopologyScopedGPUDevices (required topology scope)    */
#define KG_DEV_CODE_PARTITIONED 5u       /* ErrInsufficientPartitionedDevice (partitions honored)                */
#define KG_DEV_CODE_NO_PARTITION 6u      /* ErrNodeMissingGPUPartitionTable (partitions honored)                 */
#define KG_DEV_CODE_PART_COUNT 7u        /* ErrUnsupportedGPURequests: no partition of that GPU count (honored)  */
#define KG_DEV_CODE_NO_TREE 8u           /* ErrNodeMissingGPUDeviceTopologyTree (required topology scope)        */
#define KG_DEV_CODE_MULTI_SHARED 9u      /* ErrUnsupportedMultiSharedGPU (required topology scope)               */
#define KG_DEV_CODE_NUMA_SCOPED 10u      /* ErrInsufficientNUMAScopedDevices (topology_hint.go:34): the NUMA hint
                                            provider found fewer GPUs in a NUMA mask than requested             */
#define KG_DEV_CODE_NO_TEMPLATE 11u      /* ErrNoMatchedGPUSharedResourceTemplate (allocator_gpu.go:40,142-143)  */
#define KG_ST_RSV_AFFINITY 0x04000000u     /* ErrReasonReservationAffinity (reservation/plugin.go:366-368)  */
#define KG_ST_RSV_NODE 0x08000000u         /* "Insufficient <r> by node" (reservation/plugin.go:498-525)    */
#define KG_ST_RSV_RESERVATION 0x10000000u  /* reservation-level reasons / no reservation meets the pod      */
#define KG_ST_RSV_MASK 0x1C000000u
#define KG_ST_QUOTA 0x20000000u            /* ElasticQuota PreFilter: "Insufficient quotas" / non-preemptible
                                              (pod-level, reported on every node)                       */
#define KG_ST_DEV_RSV 0x40000000u          /* "Reservation(s) Insufficient gpu devices": the pod must allocate from a
                                            * matched reservation and none fits (deviceshare/reservation.go:404-406) */
#define KG_ST_UNSUPPORTED 0x80000000u /* pair needs the host path (e.g. cpuset binding)        */
/* The bits above whose status is UnschedulableAndUnresolvable in the reference (preemption cannot help on that node):
 * KG_ST_NUMA_CONFLICT (nodenumaresource/plugin.go:380), KG_ST_NUMA_CPU_TOPO (:403), KG_ST_NUMA_CPU_BIND (:342, :413,
 * :418) and KG_ST_DEV_NO_DEVICE (deviceshare/devicehandler_gpu.go:43). kg_eval_feasible with this fail_mask gives the
 * nodes where preemption might help. KG_ST_NODE_EXCLUDED is left out: the host knows which of its own Filters was
 * unresolvable. The DeviceShare reason is a 4-bit code, not a bit per reason: KG_ST_DEV_NO_DEVICE is also the low half's
 * bit 1 of the allocator codes 3, 6, 7, 10 and 11, of which KG_DEV_CODE_GPU_DEVICES (3) is plain Unschedulable in the
 * reference (allocator_gpu.go:334), and the unresolvable codes 8 and 9 carry no bit of the mask. On pairs with a GPU
 * allocator code the mask is therefore approximate; a caller that needs them exact reads KG_ST_DEV_CODE of
 * kg_eval_verify's word. */
#define KG_ST_UNRESOLVABLE_MASK 0x02620000u

typedef struct kg_ctx kg_ctx;   /* one per device per scheduler profile */
typedef struct kg_snap kg_snap; /* device-resident node snapshot (one shard) */
typedef struct kg_pods kg_pods; /* device-resident pending-pod batch + result buffers */

/* Plugin arguments that shape the arithmetic (pkg/scheduler/apis/config/types.go:31-435 after
 * v1 defaulting, pkg/scheduler/apis/config/v1/defaults.go:100-163). */
typedef struct kg_config {
    uint32_t plugins;      /* KG_PLUGIN_* */
    int64_t weight_nrf;    /* score plugin weights (config/manager/scheduler-config.yaml:87-98) */
    int64_t weight_la;
    int64_t weight_numa;
    /* NodeResourcesFit LeastAllocated scoringStrategy weights, resources {cpu, memory, scalar0, scalar1};
     * 0 = resource not listed. */
    int64_t nrf_w_cpu, nrf_w_mem, nrf_w_sc[KG_NSCALAR];
    /* LoadAwareScheduling */
    uint32_t la_score_enabled;      /* scoreWeights != nil (load_aware.go:113-116)              */
    uint32_t la_filter_expired;     /* FilterExpiredNodeMetrics (load_aware.go:199)             */
    uint32_t la_schedule_expired;   /* EnableScheduleWhenNodeMetricsExpired (load_aware.go:201) */
    uint32_t la_score_prod;         /* ScoreAccordingProdUsage (load_aware.go:256)              */
    int64_t la_w[KG_LA_R];          /* ResourceWeights by vectorizer index {cpu, memory}        */
    int64_t la_dominant_w;          /* DominantResourceWeight                                   */
    /* NodeNUMAResource LeastAllocated ScoringStrategy (node score) and NUMAScoringStrategy (hints). */
    int64_t numa_w_cpu, numa_w_mem;
    int64_t numa_hint_w_cpu, numa_hint_w_mem;
    /* DeviceShare / Reservation score plugin weights (config/manager/scheduler-config.yaml:91-96) and
     * DeviceShare LeastAllocated weights over {gpu-core, gpu-memory-ratio, gpu-memory}, 0 = resource
     * not listed (defaults ratio 1, memory 1: pkg/scheduler/apis/config/v1/defaults.go:254-277). */
    int64_t weight_dev;
    int64_t weight_rsv;
    int64_t dev_w[KG_DEV_R];
    /* ScoringStrategy type MostAllocated instead of LeastAllocated (nodenumaresource/most_allocated.go,
     * deviceshare/scoring.go:283-308): NodeNUMAResource node score, its NUMA hint score, DeviceShare. */
    uint32_t numa_most_allocated;
    uint32_t numa_hint_most_allocated;
    uint32_t dev_most_allocated;
    /* NodeResourcesFit scoringStrategy per resource: bit r set = MostAllocated for resource r of {cpu,
     * memory, scalar0, scalar1} (all bits: upstream's MostAllocated strategy; a mix: the per-resource
     * types of NodeResourcesFitPlus, noderesourcefitplus/node_resource_fit_plus_utils.go:58-86). */
    uint32_t nrf_most_allocated;
    /* Scalar resources left out of the fit checks (bit k: scalar k), from NodeResourcesFitArgs
     * IgnoredResources / IgnoredResourceGroups and the Reservation plugin's ignored resources
     * (reservation/plugin.go:897-909: extended resources only, never the native ones). */
    uint32_t nrf_ignored_scalars;
    uint32_t rsv_ignored_scalars;
} kg_config;

/* Node snapshot, struct-of-arrays host columns, n_nodes entries each (caller-owned, copied). */
/* ---- cpuset binding (NodeNUMAResource with LSE/LSR pods) ----------------------- */
#define KG_MAX_CPUS 256
/* CPU bind policies (apis/scheduling/config CPUBindPolicy) and exclusive policies (CPUExclusivePolicy). */
#define KG_CPU_BIND_NONE 0u
#define KG_CPU_BIND_FULL_PCPUS 1u
#define KG_CPU_BIND_SPREAD_BY_PCPUS 2u
#define KG_CPU_EXCL_NONE 0u
#define KG_CPU_EXCL_PCPU_LEVEL 1u
#define KG_CPU_EXCL_NUMA_NODE_LEVEL 2u
/* Node CPU bind policy (apis/extension NodeCPUBindPolicy via GetNodeCPUBindPolicy). */
#define KG_NODE_CPU_BIND_NONE 0u
#define KG_NODE_CPU_BIND_FULL_PCPUS_ONLY 1u
#define KG_NODE_CPU_BIND_SPREAD_BY_PCPUS 2u
/* NUMA allocate strategy of the accumulator (NUMAMostAllocated / NUMALeastAllocated). */
#define KG_NUMA_MOST_ALLOCATED 0u
#define KG_NUMA_LEAST_ALLOCATED 1u
/* CPU topology of one node (nodenumaresource/cpu_topology.go CPUTopology). CPU ids are 0..n_cpus-1; core,
 * NUMA node and socket ids are dense ranks of the reference's ids (order preserved: the accumulator breaks
 * ties by id). n_sockets == 0 (or any count 0): no valid topology (CPUTopology.IsValid). */
typedef struct kg_cpu_topo {
    uint16_t n_cpus, n_cores, n_nodes, n_sockets;
    uint8_t core[KG_MAX_CPUS];
    uint8_t numa[KG_MAX_CPUS];
    uint8_t socket[KG_MAX_CPUS];
} kg_cpu_topo;
/* CPUs already allocated on a node (NodeAllocation.allocatedCPUs): per CPU its RefCount (0 = free) and the
 * CPUExclusivePolicy of the allocation that holds it. */
typedef struct kg_cpu_alloc {
    uint8_t ref[KG_MAX_CPUS];
    uint8_t excl[KG_MAX_CPUS];
} kg_cpu_alloc;

/* One takeCPUs / takePreferredCPUs request (nodenumaresource/cpu_accumulator.go:30-246). */
typedef struct kg_cpuset_request {
    uint32_t topo;          /* index into the topologies of the call                                   */
    int32_t alloc;          /* index into the allocations of the call, -1 = nothing allocated          */
    uint64_t avail[4];      /* allocatable CPUs (NodeAllocation.getAvailableCPUs)                       */
    uint64_t preferred[4];  /* preferred CPUs (takePreferredCPUs); used when has_preferred               */
    int32_t needed;         /* numCPUsNeeded                                                            */
    int32_t max_ref;        /* TopologyOptions.MaxRefCount (>= 1)                                       */
    int32_t bind;           /* KG_CPU_BIND_*                                                            */
    int32_t excl;           /* the pod's KG_CPU_EXCL_*                                                  */
    int32_t strategy;       /* KG_NUMA_MOST_ALLOCATED / KG_NUMA_LEAST_ALLOCATED                         */
    int32_t has_preferred;
} kg_cpuset_request;

/* One GPU partition (apis/extension/device_share.go:221-227 GPUPartition). */
#define KG_GPU_NO_SCOPE 0xFFu
#define KG_GPU_HONOR 0x100u
#define KG_GPU_TREE 0x200u
#define KG_GPU_TMPL_SHIFT 12 /* dev_part bits 12-15: the node's shared-resource template key (KG_GPU_TMPL_NONE = none) */
#define KG_GPU_TMPL_NONE 15u
#define KG_ZONE_RECORD_SHIFT 8 /* numa_zone_status: zone z has an allocation record (node_allocation.go:145-154) */
#define KG_GPU_MAX_TABLES 16
#define KG_GPU_MAX_PARTS 1024
typedef struct kg_gpu_partition {
    uint8_t table;           /* partition table index (dev_part - 1)                                   */
    uint8_t n_gpus;          /* the table key: number of GPUs (1..8)                                   */
    uint8_t minors;          /* MinorsHash: bit m = minor m                                            */
    uint8_t pad_;
    int32_t alloc_score;     /* AllocationScore                                                        */
    int64_t ring_bw;         /* RingBusBandwidth in bytes, -1 = none                                   */
} kg_gpu_partition;

typedef struct kg_node_columns {
    /* upstream NodeInfo (k8s v1.35.6): Allocatable / Requested / NonZeroRequested / len(Pods) */
    const int64_t *alloc_cpu, *alloc_mem, *alloc_eph, *alloc_pods;
    const int64_t *req_cpu, *req_mem, *req_eph, *num_pods;
    const int64_t *nz_cpu, *nz_mem;
    const int64_t *sc_alloc[KG_NSCALAR], *sc_req[KG_NSCALAR];
    /* LoadAwareScheduling: EstimateNode allocatable, thresholds of the node's filter profile after
     * its custom-threshold annotation (helper.go:83-121), and the estimated usage of existing pods
     * returned by GetNodeMetricAndEstimatedOfExisting (pod_assign_cache.go:163-201) for the filter
     * (non-prod / prod pod) and the score (non-prod / prod pod). */
    const uint32_t* la_flags;
    const int64_t* la_alloc[KG_LA_R];
    const int64_t* la_thr_usage[KG_LA_R];
    const int64_t* la_thr_prod[KG_LA_R];
    const int64_t* la_thr_agg[KG_LA_R];
    const int64_t* la_fbase_np[KG_LA_R];
    const int64_t* la_fbase_prod[KG_LA_R];
    const int64_t* la_sbase_np[KG_LA_R];
    const int64_t* la_sbase_prod[KG_LA_R];
    /* NodeNUMAResource */
    const uint32_t* numa_policy;        /* KG_NUMA_* after merging node label and kubelet policy     */
    const uint32_t* numa_zones;         /* number of NUMA zones with resources (0..KG_MAX_ZONES)     */
    const double* cpu_amp_ratio;        /* cpu amplification ratio (<= 1: none)                      */
    const int64_t* cpuset_alloc_milli;  /* milli-cpu allocated as cpusets                            */
    const int64_t* zone_cpu[KG_MAX_ZONES];      /* zone totals (amplified, util.go:101-124)          */
    const int64_t* zone_mem[KG_MAX_ZONES];
    const int64_t* zone_cpu_used[KG_MAX_ZONES]; /* zone allocated                                     */
    const int64_t* zone_mem_used[KG_MAX_ZONES];
    /* DeviceShare: the node's GPU minors (nodeDevice of deviceshare/device_cache.go). dev_minors < 0:
     * the node has no Device object (Filter passes, Score 0: deviceshare/plugin.go:398-401,
     * scoring.go:58-61); otherwise minors 0..dev_minors-1. dev_total / dev_free are row-major
     * [node][KG_DEV_R][KG_DEV_MINORS] with 0 <= free <= total (NULL = no DeviceShare data). */
    const int32_t* dev_minors;
    const int64_t* dev_total;
    const int64_t* dev_free;
    /* NUMA node shared status per zone, 2 bits each (0 idle, 1 single, 2 shared; NUMANodeSharedStatus,
     * nodenumaresource/node_allocation.go:52-68) for the Required exclusive policy of pods with a
     * pod-level NUMA policy (NULL = all idle). */
    const uint32_t* numa_zone_status;  /* 2 bits per zone NUMANodeSharedStatus; bit KG_ZONE_RECORD_SHIFT + z: the
                                        * NodeAllocation holds an allocatedResources record for zone z */
    /* cpuset binding (NodeNUMAResource, LSE/LSR pods; all may be NULL = no CPU topology anywhere):
     * cpu_topo[i] indexes cpu_topos (-1 = the node has no CPU topology: ErrInvalidCPUTopology for a
     * cpuset-binding pod); cpu_alloc[i] = the node's allocated CPUs (NULL = none). cpuset_alloc_milli must
     * then equal 1000 x the CPUs with RefCount > 0. cpu_max_ref (NULL = 1), cpu_bind_policy
     * (KG_NODE_CPU_BIND_*, GetNodeCPUBindPolicy) and cpu_strategy (KG_NUMA_MOST/LEAST_ALLOCATED,
     * GetNUMAAllocateStrategy) are per node. */
    const int32_t* cpu_topo;
    const kg_cpu_topo* cpu_topos;
    uint32_t n_cpu_topos;
    const kg_cpu_alloc* cpu_alloc;
    const uint8_t* cpu_max_ref;
    const uint8_t* cpu_bind_policy;
    const uint8_t* cpu_strategy;
    /* DeviceShare GPU topology and partitions (deviceshare/allocator_gpu.go:72-451, allocator_gpu_helper.go
     * :150-275; all may be NULL = no tree, no partition table, Prefer policy):
     * dev_topo[i]: byte m = GPU minor m's place in the topology tree (GetGPUTopologyScope): high nibble the
     *   rank of its NUMA node id (numeric order), low nibble the rank of its (NUMA node, PCIe id) pair
     *   (PCIe ids in string order within a NUMA node); each rank < 8 (the device reads 3 bits of each nibble;
     *   more than 8 NUMA nodes or pairs is unsupported); KG_GPU_NO_SCOPE = the minor is in no NUMA / PCIe scope;
     * dev_part[i]: bits 0-7 = 1 + the node's partition table in gpu_parts (0 = none: GetGPUPartitionIndexer of
     *   the Device annotation, else the designated table of the node's GPU model), KG_GPU_HONOR = the
     *   GPUPartitionPolicy label is Honor, KG_GPU_TREE = the node has a topology tree (every GPU DeviceInfo
     *   carries a Topology), bits 12-15 (KG_GPU_TMPL_SHIFT) = the index of the node's GPU shared-resource
     *   template key buildGPUSharedResourceTemplatesKey(vendor, model) among the configured keys, or
     *   KG_GPU_TMPL_NONE when the configuration holds no templates for that key;
     * gpu_parts: every partition of every table (kg_gpu_partition), grouped by table, then GPU count, then
     *   AllocationScore ascending; within a group in the table's order (GetGPUPartitionIndexer). */
    const uint64_t* dev_topo;
    const uint32_t* dev_part;
    const struct kg_gpu_partition* gpu_parts;
    uint32_t n_gpu_parts;
    /* DeviceShare NUMA topology (deviceshare/numa_topology.go:43-100, NUMATopology.deviceToNodeID; NULL = every
     * minor without a topology): nibble m of dev_numa[i] = GPU minor m's NUMA node id (0..KG_MAX_ZONES-1, the NRT zone of
     * that id; the upload rejects larger ids), KG_GPU_NUMA_ANY = its Topology.NodeID is -1 (in every NUMA mask, in no NUMA scope), KG_GPU_NUMA_NONE =
     * no Topology (left out whenever a NUMA affinity restricts the allocation, device_allocator.go:155-159).
     * GPU pods on nodes whose NUMA policy is not None join the topology manager's hint merge with these
     * (deviceshare/topology_hint.go:40-290). */
    const uint32_t* dev_numa;
    /* The cpuset pods behind numa_zone_status (NodeAllocation.singleNUMANode / sharedNode, node_allocation.go:111-143):
     * byte z (z < KG_MAX_ZONES) = pods whose CPUs lie in NUMA node z only, byte KG_MAX_ZONES + z = pods whose CPUs span z
     * and another node (saturating at 255). A cpuset Release (kg_unreserve) takes its pod out again, so the statuses it
     * leaves follow from these counts. NULL: one pod per non-idle status (single -> 1 / 0, shared -> 0 / 1); when given,
     * the 2-bit statuses of numa_zone_status are derived from them. */
    const uint64_t* numa_zone_pods;
    /* 1: a reservation on the node (matched by the pod or not) holds a NUMA or cpuset allocation (its reserve pod's
     * resource status). NodeNUMAResource's RestoreReservation (nodenumaresource/reservation.go:188-262) gives such
     * allocations back to the owners of a matched reservation and the double-counted owner usage of unmatched ones,
     * in the hints (resource_manager.go:131-160), tryAllocateFromReusable / tryAllocateFromNode (plugin.go:428-439,
     * 807-851) and the Reserve; the device does not follow that restore, so every pair on such a node where the
     * plugin reads it (the pod binds CPUs there, or the merged NUMA policy is not None) is KG_ST_UNSUPPORTED and the
     * sequential calls (kg_replay, kg_batch_schedule, kg_reserve, kg_assume*) refuse those pods (KG_UNSUPPORTED).
     * NULL = none (ABI 12). */
    const uint8_t* rsv_numa;
} kg_node_columns;
#define KG_GPU_NUMA_ANY 0xEu
#define KG_GPU_NUMA_NONE 0xFu

/* Mutable node state that Assume/Forget change; used to read a snapshot back after kg_replay. */
typedef struct kg_node_state {
    int64_t *req_cpu, *req_mem, *req_eph, *num_pods, *nz_cpu, *nz_mem;
    int64_t* sc_req[KG_NSCALAR];
    int64_t *la_fbase_np[KG_LA_R], *la_fbase_prod[KG_LA_R];
    int64_t *la_sbase_np[KG_LA_R], *la_sbase_prod[KG_LA_R];
    int64_t *zone_cpu_used[KG_MAX_ZONES], *zone_mem_used[KG_MAX_ZONES];
    int64_t* dev_free; /* [node][KG_DEV_R][KG_DEV_MINORS] */
    int64_t* cpuset_alloc_milli;
    kg_cpu_alloc* cpu_alloc; /* [node] (nodes without a CPU topology: zeros) */
    uint32_t* numa_zone_status; /* NUMANodeSharedStatus, 2 bits per zone (a cpuset Reserve changes it) */
    uint64_t* numa_zone_pods;   /* kg_node_columns.numa_zone_pods */
} kg_node_state;

/* Pending pods, struct-of-arrays host columns (caller-owned, copied). */
typedef struct kg_pod_columns {
    const int64_t *req_cpu, *req_mem, *req_eph; /* PodRequests: milli-cpu, bytes, bytes            */
    const int64_t* sc_req[KG_NSCALAR];
    const int64_t *nz_cpu, *nz_mem;             /* non-zero requests (100m / 200Mi defaults)        */
    const int64_t* la_est[KG_LA_R];             /* DefaultEstimator.EstimatePod (estimator/default_estimator.go:57-120) */
    const uint32_t* flags;                      /* KG_POD_*                                         */
    const uint32_t* numa_policy;                /* pod NUMA topology policy annotation, KG_NUMA_*   */
    /* DeviceShare GPURequirements (deviceshare/utils.go:516-545, devicehandler_gpu.go:53-96):
     * per-instance request [pod][KG_DEV_R], number of GPUs (0 = no GPU request: PreFilter Skip) and
     * the keys present in requestsPerGPU (bit KG_DEV_*). */
    const int64_t* dev_req;
    const uint32_t* dev_count;
    const uint32_t* dev_keys;
    /* ElasticQuota: quota index (-1 = none: PreFilter Skip) and the keys of PodRequests masked by the
     * quota's Max names (bit r of KG_QUOTA_R), elasticquota/plugin.go:279-281. */
    const int32_t* quota;
    const uint32_t* quota_keys;
    /* Reservation owner-match class (-1 = the pod matches no reservation): pods of one class match
     * the same reservations (reservation/transformer.go:233-240, checkReservationMatchedOrIgnored). */
    const int32_t* rsv_class;
    /* GPURequirements beyond the request (deviceshare/utils.go:516-545; NULL = none): KG_GPU_POD_* flags and
     * the GPUPartitionSpec RingBusBandwidth in bytes (read when KG_GPU_POD_RING_BW is set). */
    const uint32_t* dev_flags;
    const int64_t* dev_ring_bw;
    /* candidateGPUSharedResourceTemplates of a KG_GPU_POD_TEMPLATE pod (deviceshare/utils.go:540-547,
     * gpu_shared_resource_templates_cache.go:41-62): 2 bits per template key k < KG_GPU_TMPL_NONE (the node's
     * key in dev_part bits 12-15) = how many templates of key k the pod's requestsPerGPU matched: 0 none, 1 one,
     * 2 several. NULL = no template pods. */
    const uint32_t* dev_tmpl;
} kg_pod_columns;

/* Verify-mode outputs, [n_pods][n_nodes] row-major, caller-allocated host buffers (NULL = skip). */
typedef struct kg_verify_out {
    uint32_t* status;     /* KG_ST_* bits per plugin; 0 = feasible                         */
    int64_t* score_nrf;   /* NodeResourcesFit score (0 when infeasible or plugin disabled)  */
    int64_t* score_la;    /* LoadAwareScheduling score                                      */
    int64_t* score_numa;  /* NodeNUMAResource score                                         */
    int64_t* total;       /* Σ weight·score, -1 when infeasible                             */
    int8_t* numa_zone;    /* NUMA allocation the Reserve would make: -1 none, 0..3 one zone,
                             0x40 | zone mask for a split over several zones, 0x20 | bits when
                             the Reserve fails (BestEffort: bits = KG_ST_NUMA_INSUF_* >> 12,
                             0x08 the cpuset take), 0x30 | KG_DEV_CODE_* when the GPU allocation
                             under the Reserve's NUMA affinity fails (a GPU pod on a BestEffort node).
                             A GPU pod's Reserve allocates its minors inside the NUMA nodes of this
                             affinity (deviceshare/plugin.go:585-600) */
    int64_t* score_dev;   /* DeviceShare Score before NormalizeScore (0 when infeasible)    */
    int64_t* score_rsv;   /* Reservation Score before NormalizeScore (1000 on the preferred
                             node, reservation/scoring.go:40,191-198; 0 when infeasible)     */
} kg_verify_out;

/* ElasticQuota table, [quota][KG_QUOTA_R] values with per-quota key masks (bit r = key present).
 * used / used_limit: the PreFilter's state.used / state.usedLimit (runtime when EnableRuntimeQuota,
 * else max; elasticquota/plugin.go:274-284); min / np_used: CalculateInfo.Min and the non-preemptible
 * used (:286-293). Quotas are flat (no parent check: EnableCheckParentQuota=false). */
typedef struct kg_quota_columns {
    const int64_t *used, *used_limit, *min, *np_used;
    const uint32_t *used_keys, *limit_keys, *min_keys, *np_used_keys;
} kg_quota_columns;

/* Restored NodeInfo of one node as pods of one owner class see it, after the Reservation transformer
 * (reservation/transformer.go:740-811): the unmatched reservations' double-counted Allocated returned
 * (updateNodeInfoRequestedForUnmatched :918-935) and the matched reserve pods removed
 * (restoreMatchedReservation :855-878). The snapshot columns hold the view of pods that match nothing
 * on the node (every reservation unmatched). */
typedef struct kg_rsv_view {
    uint32_t node;                       /* local node index                                         */
    uint32_t cls;                        /* owner-match class (kg_pod_columns.rsv_class)             */
    uint32_t first, count;               /* matched reservations: kg_rsv_info[first, first + count)  */
    int64_t req[KG_RSV_R];               /* restored Requested                                       */
    int64_t nz_cpu, nz_mem, num_pods;    /* restored NonZeroRequested and len(Pods)                  */
    int64_t pod_requested[KG_RSV_R];     /* nodeRState.podRequested (after the unmatched correction) */
    int64_t r_allocated[KG_RSV_R];       /* nodeRState.rAllocated: Σ Allocated of matched reservations */
    /* DeviceShare: kg_rsv_dev index of the GPU minors a pod of this class allocates from outside its
     * reservations (unmatched reservations' used and matched reservations' allocatable given back:
     * deviceshare/plugin.go:397-419, reservation.go:94-117); -1 = the node's own minors. */
    int32_t dev_base;
    uint32_t pad_;
} kg_rsv_view;

/* One matched reservation (frameworkext.ReservationInfo). */
typedef struct kg_rsv_info {
    uint32_t policy;                     /* KG_RSV_*                                                 */
    uint32_t names;                      /* bit r: resource r in ResourceNames (keys of Allocatable) */
    uint32_t allocate_once;              /* IsAllocateOnce (apis/extension/reservation.go:167)       */
    int32_t dev;                         /* kg_rsv_dev index of the GPU minors a pod allocates from this
                                          * reservation (tryAllocateFromReusable, deviceshare/reservation.go
                                          * :344-410); -1 = it reserves no GPU                         */
    int64_t order;                       /* LabelReservationOrder, 0 = none; |order| < 2^31          */
    int64_t allocatable[KG_RSV_R], allocated[KG_RSV_R], reserved[KG_RSV_R];
    int64_t max_pods;                    /* "pods" in Allocatable, -1 = absent                       */
    int64_t allocated_pods;              /* len(AssignedPods)                                        */
    uint32_t rid;                        /* the reservation's id on its node: the copies of one reservation
                                          * in the views of several classes share it (a Reserve into it
                                          * updates all of them)                                       */
    uint32_t allocated_keys;             /* bit 0 / 1: Allocated holds a cpu / memory key (0 while nil):
                                          * GetNonZeroRequestForResource of the unmatched correction   */
    uint32_t dev_minors;                 /* the GPU minors the reservation reserves (bit m; ABI 12): a pod allocating
                                          * from it takes them first (tryAllocateFromReusable's preferred set,
                                          * deviceshare/reservation.go:308; defaultAllocateDevices ->
                                          * sortDeviceResourcesByMinor, device_resources.go:187-209)      */
    uint32_t pad_;
} kg_rsv_info;

/* GPU minors as one restore sees them (nodeDevice.calcFreeWithPreemptible / filter, deviceshare/
 * device_cache.go:322-410): total and free per resource (KG_DEV_CORE / _RATIO / _MEM) and minor; a minor
 * outside the allocation's reach has total 0 and free 0. */
typedef struct kg_rsv_dev {
    int64_t total[KG_DEV_R][KG_DEV_MINORS];
    int64_t free[KG_DEV_R][KG_DEV_MINORS];
} kg_rsv_dev;

/* ------------------------------------------------------------------------------------------------ */
int kg_abi_version(void);
const char* kg_status_string(kg_status s);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int kg_device_count(void);

kg_status kg_open(int device, kg_ctx** out);
kg_status kg_close(kg_ctx* ctx);
/* Message of the last failed call on ctx (empty string if none). Valid until the next call. */
const char* kg_last_error(const kg_ctx* ctx);
/* Wait for all work queued on the context's stream. */
kg_status kg_sync(kg_ctx* ctx);

/* Snapshot of n_nodes nodes whose global snapshot indices are [index_base, index_base + n_nodes). */
kg_status kg_snapshot_create(kg_ctx* ctx, const kg_config* cfg, uint32_t n_nodes, uint32_t index_base,
                             kg_snap** out);
kg_status kg_snapshot_upload(kg_snap* snap, const kg_node_columns* cols);
/* Replace rows[i] (local index) with entry i of cols (each column has n entries): the informer-event
 * deltas of one scheduling cycle in one call (one staged copy + one scatter launch on the device). */
kg_status kg_snapshot_update_rows(kg_snap* snap, const uint32_t* rows, uint32_t n, const kg_node_columns* cols);
/* Generation of the snapshot: bumped by every call that changes its contents (upload, update_rows,
 * kg_assume / kg_forget and their _ext forms, kg_replay, quota and reservation uploads). A caller that
 * stamps its host cache with it can tell whether the device has seen every delta (k8s UpdateSnapshot's
 * NodeInfo.Generation scheme; the host side is koordinator_amd.cluster). */
kg_status kg_snapshot_generation(kg_snap* snap, uint64_t* out);
kg_status kg_snapshot_read_state(kg_snap* snap, kg_node_state* out);
/* ElasticQuota table (KG_PLUGIN_QUOTA): n_quotas entries, copied; Reserve updates used / np_used. */
kg_status kg_snapshot_upload_quotas(kg_snap* snap, const kg_quota_columns* cols, uint32_t n_quotas);
/* Read back used / np_used (and their key masks) after kg_replay / kg_assume_ext. */
kg_status kg_snapshot_read_quotas(kg_snap* snap, int64_t* used, uint32_t* used_keys, int64_t* np_used,
                                  uint32_t* np_used_keys);
/* Reservation views of this snapshot (KG_PLUGIN_RSV), replacing any earlier upload. Views of one
 * class must name distinct nodes; at most 64 classes and 8 reservations per view. */
kg_status kg_snapshot_upload_reservations(kg_snap* snap, const kg_rsv_view* views, uint32_t n_views,
                                          const kg_rsv_info* infos, uint32_t n_infos, const kg_rsv_dev* devs,
                                          uint32_t n_devs);
/* DeviceShare restore inputs of the reservations that hold GPUs (deviceshare/reservation.go:139-198 RestoreReservation
 * reads them from nodeDevice every cycle): per such node one entry with rid -1 whose `a` is the node's deviceUsed, and
 * one entry per GPU-holding reservation on it (kg_rsv_info.rid): `a` = its reserve pod's allocation (allocatable),
 * `b` = its assigned pods' allocations on those minors (allocated), its policy and assigned pod count. With them
 * kg_replay, kg_batch_schedule and kg_reserve / kg_unreserve follow a Reserve into such a node on the device (the
 * node's used, the reservation the pod joins, and the restore tables of the record, the views and the reservations,
 * rebuilt as transformer.go:740-935 + reservation.go:139-198,278-380 would); without them those calls refuse
 * (KG_UNSUPPORTED) or mark the node's views stale. kg_snapshot_upload_reservations / kg_snapshot_update_views drop
 * the inputs (upload them again after). */
typedef struct kg_rsv_gpu {
    uint32_t node;           /* local node index                                                        */
    int32_t rid;             /* kg_rsv_info.rid, -1 = the node's entry                                  */
    uint32_t policy;         /* KG_RSV_* (reservation entries)                                          */
    uint32_t allocated_pods; /* len(AssignedPods) (reservation entries)                                 */
    int64_t a[KG_DEV_R][KG_DEV_MINORS];
    int64_t b[KG_DEV_R][KG_DEV_MINORS];
} kg_rsv_gpu;
kg_status kg_snapshot_upload_rsv_gpu(kg_snap* snap, const kg_rsv_gpu* entries, uint32_t n);
/* Replace the views (with their reservations and GPU restore tables) of the nodes in nodes[0, n_nodes) by views[0, n_views)
 * (each naming one of those nodes; a listed node without views loses its views); every other node keeps its views.
 * The incremental form of kg_snapshot_upload_reservations for the nodes a Reserve / Unreserve or an event changed
 * (the Reservation transformer's per-node restore, reservation/transformer.go:740-935): it clears their staleness. */
kg_status kg_snapshot_update_views(kg_snap* snap, const uint32_t* nodes, uint32_t n_nodes, const kg_rsv_view* views,
                                   uint32_t n_views, const kg_rsv_info* infos, uint32_t n_infos, const kg_rsv_dev* devs,
                                   uint32_t n_devs);
kg_status kg_snapshot_destroy(kg_snap* snap);

kg_status kg_pods_create(kg_ctx* ctx, uint32_t capacity, kg_pods** out);
kg_status kg_pods_upload(kg_pods* pods, const kg_pod_columns* cols, uint32_t n_pods);
/* Lanes the next plain (non config-5) kg_eval_select / kg_shard_select of this batch launches: one per pod, or one
 * per distinct input row when the upload found equal rows and evaluating only their representatives at least halves the
 * 64-lane waves (the duplicates' keys and status are copied from their representative on the device; results are the
 * same). fast_lanes: the leading lanes on the float64 fast path. Either pointer may be NULL. Diagnostics only. */
kg_status kg_pods_select_lanes(const kg_pods* pods, uint32_t* lanes, uint32_t* fast_lanes);
/* The fast lanes among them on this snapshot: kg_pods_select_lanes' count, or 0 when the snapshot's configuration is
 * outside the fast path's domain (a per-resource weight above 4096, a LoadAware weight sum above 4096, a MostAllocated
 * strategy, ignored scalars) or KG_SELECT_INT=1 / the exact mode sends every lane to the integer path. Diagnostics only. */
kg_status kg_select_fast_lanes(const kg_snap* snap, const kg_pods* pods, uint32_t* fast_lanes);
/* Per-pod candidate node sets: the nodes each pod of the uploaded batch may use, as the scheduler narrowed them before
 * koord's plugins run (nodeSelector and required node affinity, taints and tolerations, spec.nodeName,
 * NodeUnschedulable, PodTopologySpread, a nominated node, a PreFilterResult). A pair (pod j, node i) with i outside j's
 * set fails a Filter that runs before every koord plugin and after the ElasticQuota PreFilter gate:
 *   kg_eval_select    (plain snapshots, k = 1..4) keys are the top-k over the candidate nodes only, an empty set gives
 *                     keys 0, and kg_result_status flags a pod only for a candidate pair (a set lane is flagged when
 *                     any candidate pair needs the host path);
 *   kg_eval_verify    an excluded pair's status is its usual word | KG_ST_NODE_EXCLUDED and its total is -1; the score
 *                     columns and numa_zone stay as they are without sets;
 *   kg_eval_diagnose  flags 0: slot 15 counts the excluded nodes (the counted word is verify's); KG_DIAG_FIRST_PLUGIN:
 *                     an excluded node's counted word is KG_ST_NODE_EXCLUDED alone (after KG_ST_QUOTA, before
 *                     KG_ST_NRF_MASK); KG_DIAG_FEASIBLE counts candidate nodes only;
 *   kg_replay         (plain snapshots) each pod's cycle picks among its candidates; out_reason carries
 *                     KG_ST_NODE_EXCLUDED when the pod has an excluded node; the batch runs one pod per launch.
 * Called after kg_pods_upload; everything is copied. A later kg_pods_upload clears the sets, sets == NULL clears them
 * too. Bits at or above n_nodes in a set's last word are ignored. KG_INVALID_ARG: no batch uploaded, a pod_set value
 * outside [-1, n_sets), n_sets > 0 with bits == NULL. An evaluating call returns KG_INVALID_ARG when its snapshot's
 * node count differs from n_nodes.
 * KG_UNSUPPORTED while the batch carries sets: every evaluating call on a snapshot with config-5 tables
 * (KG_PLUGIN_EXT: the per-pod NormalizeScore runs over the narrowed set) and kg_shard_select (the exchange of the
 * shards). kg_batch_schedule, kg_reserve, kg_assume*, kg_forget* and kg_unreserve name their node themselves and do
 * not read the sets. The symbol is new within ABI 14: a binding resolves it at load time. */
typedef struct kg_node_sets {
    const int32_t* pod_set;  /* [n_pods of the uploaded batch]; -1 = every node (no set) */
    const uint32_t* bits;    /* [n_sets][(n_nodes + 31) / 32]: bit (i & 31) of word (i >> 5) set = the node at snapshot
                                position i is a candidate. The position is the row of the node upload; index_base is
                                not added */
    uint32_t n_sets, n_nodes;
} kg_node_sets;
kg_status kg_pods_set_node_sets(kg_pods* pods, const kg_node_sets* sets /* NULL clears */);
/* Per-pod host score terms: the Score plugins that stay on the host (NodeAffinity preferred terms, TaintToleration
 * PreferNoSchedule, ImageLocality, PodTopologySpread, InterPodAffinity) hand their score lists in, and selectHost runs
 * over koord's total plus theirs. A row is one plugin's score list for one kind of pod (the preferred weights of one
 * pod template): pods the plugin scores alike share it, and a pod names up to KG_SCORE_TERMS rows.
 *   Pod j's feasible candidates are the nodes whose kg_eval_verify status word is 0 (KG_ST_NODE_EXCLUDED of a
 *   candidate node set included). For term t with row r, m = max raw[r][i] over them; the term's value on a feasible
 *   candidate i is
 *     KG_SCORE_RAW                raw[r][i]
 *     KG_SCORE_NORMALIZE          m == 0 ? 0 : 100 * raw[r][i] / m
 *     KG_SCORE_NORMALIZE_REVERSE  m == 0 ? 100 : 100 - 100 * raw[r][i] / m
 *   in integer division (DefaultNormalizeScore(100, reverse), pkg/scheduler/frameworkext/normalize_score.go:24-52 and
 *   upstream's helper of the same shape). The pair's total is koord's total + the sum over t of weight[r] x value.
 *   kg_eval_select    (plain snapshots, k = 1..4) keys are the top-k of that total over the feasible candidates; ties
 *                     go to the lowest snapshot index as before; kg_result_status flags a pod with terms as it flags a
 *                     set lane (when any candidate pair needs the host path);
 *   kg_eval_verify    total of a feasible candidate pair is that total; every other column and every infeasible pair
 *                     are as without terms;
 *   kg_eval_diagnose, kg_eval_feasible  Filter only: they accept the batch and return what they return without terms.
 * Called after kg_pods_upload; everything is copied. A later kg_pods_upload clears the terms, scores == NULL clears
 * them too. Sets and terms are independent: clearing one keeps the other. KG_INVALID_ARG: no batch uploaded, a row id
 * outside [-1, n_rows), a raw value outside [0, KG_SCORE_RAW_MAX], an unknown mode, a weight above 2^20. An evaluating
 * call (select, verify) returns KG_INVALID_ARG when its snapshot's node count differs from n_nodes, or when the
 * snapshot's sum of plugin weights x 100 plus the largest per-pod bound of the terms (sum over t of weight x (100, or
 * the row's largest raw for KG_SCORE_RAW)) could reach 2^31, the total field of the packed key.
 * KG_UNSUPPORTED while the batch carries terms: kg_eval_select / kg_eval_verify on a snapshot with config-5 tables
 * (KG_PLUGIN_EXT), kg_shard_select (the maximum is global over the shards) and kg_replay. kg_batch_schedule,
 * kg_reserve, kg_assume*, kg_forget* and kg_unreserve name their node themselves and do not read the terms. The symbol
 * is new within ABI 14: a binding resolves it at load time. */
#define KG_SCORE_TERMS 4                 /* host score terms per pod */
#define KG_SCORE_RAW 0u                  /* value = raw */
#define KG_SCORE_NORMALIZE 1u            /* DefaultNormalizeScore(100, reverse=false) over the pod's feasible candidates */
#define KG_SCORE_NORMALIZE_REVERSE 2u    /* ... reverse=true */
#define KG_SCORE_RAW_MAX (1 << 20)
typedef struct kg_node_scores {
    const int32_t* pod_terms;  /* [n_pods][KG_SCORE_TERMS]: row id, -1 = unused slot */
    const int32_t* raw;        /* [n_rows][n_nodes], snapshot positions (index_base not added), 0..KG_SCORE_RAW_MAX */
    const uint32_t* mode;      /* [n_rows] KG_SCORE_* */
    const uint32_t* weight;    /* [n_rows] the plugin's weight, 0..2^20 */
    uint32_t n_rows, n_nodes;
} kg_node_scores;
kg_status kg_pods_set_node_scores(kg_pods* pods, const kg_node_scores* scores /* NULL clears */);
kg_status kg_pods_destroy(kg_pods* pods);

/* Full per-plugin Filter/Score matrix for every (pod, node) pair (the FilterPlugin/ScorePlugin
 * results the Go plugins would return). */
kg_status kg_eval_verify(kg_snap* snap, kg_pods* pods, kg_verify_out* out);
/* Filter + Score + selectHost for every pending pod against the snapshot as it is (matrix mode):
 * per pod the k best packed keys (kg_make_key), descending, 0 = no feasible node. The launch is
 * asynchronous; results stay on the device until kg_result_keys. Where the device kept one result per distinct pod row
 * (the one-launch top-1 select: by default the launch's own accumulators are that result, a few replicas of key and status
 * words per row, which the readers fold; or one key and status word per row stored by the launch's last workgroup),
 * kg_result_keys and kg_result_status copy those and fill in the rows on the host, through
 * the row table of the upload that the select ran on; both may be called any number of times, in either order.
 * Read a result before the batch's next kg_pods_upload: the upload replaces that table, and until the next select on
 * the batch both calls then fail with KG_INVALID_ARG ("no selection result") rather than serve rows of the old batch
 * through the new one's table. (A result kept per row is still served after an upload, as before: the first n_pods
 * rows of the earlier select.) kg_pods_set_node_sets / kg_pods_set_node_scores do not invalidate a result. */
kg_status kg_eval_select(kg_snap* snap, kg_pods* pods, uint32_t k);
kg_status kg_result_keys(kg_pods* pods, uint64_t* out_keys /* n_pods * k */);
/* Per-pod outcome flags of the last kg_eval_select / kg_shard_select (n_pods entries):
 *   KG_ST_UNSUPPORTED  some (pod, node) pair needs the host path (cpuset binding, a failing BestEffort
 *                      NUMA Reserve, DeviceShare with device NUMA hints, ...): the pod's keys cover only
 *                      the pairs the device decided, so the caller runs the reference plugins for it;
 *   KG_ST_QUOTA        the ElasticQuota PreFilter rejected the pod (no node evaluated, keys 0);
 *   0                  the keys are the complete Filter/Score/selectHost result. */
kg_status kg_result_status(kg_pods* pods, uint32_t* out_status);
/* FitError diagnosis of unschedulable pods: per requested pod, the number of nodes of this snapshot that fail with
 * each Filter reason (ABI 14). The framework's FitError.Error() prints "0/N nodes are available: 8 Insufficient cpu,
 * 3 node(s) cpu usage exceed threshold." from exactly these counts (upstream k8s.io/kubernetes
 * pkg/scheduler/framework/types.go FitError.Error: the reasons histogram of Diagnosis.NodeToStatus, "%v %v" items
 * sorted as strings and joined by ", "; koordinator's tables carry the text, e.g.
 * coscheduling/core/network_topology_workflow_test.go:1255, core_test.go:569).
 *   rows[t]  a pod index of the uploaded batch; rows may repeat and come in any order; output row t belongs to
 *            rows[t]. rows == NULL: every pod in batch order (n_rows must equal the batch size).
 *   out_counts[t * KG_DIAG_SLOTS + b], b in 0..31: nodes whose counted status word has bit b (KG_ST_*) set;
 *            slot KG_DIAG_DEV_CODE0 + c, c in 1..15: nodes whose DeviceShare code (KG_ST_DEV_CODE) is c (slot 32
 *            stays 0); slot KG_DIAG_FEASIBLE: nodes whose counted word is 0; slots 49..63 are written as 0.
 *   flags    0: the counted word is the pair's status word as kg_eval_verify reports it (every failing plugin's
 *            bits). KG_DIAG_FIRST_PLUGIN: that word masked to its first non-empty group in the framework's order,
 *            which stops at a node's first failing plugin: the ElasticQuota PreFilter gate (KG_ST_QUOTA),
 *            KG_ST_NODE_EXCLUDED (a batch with candidate node sets: the host's Filters ran before koord's), then the
 *            filter order of config/manager/scheduler-config.yaml:69-74: KG_ST_NRF_MASK, KG_ST_LA_MASK,
 *            KG_ST_NUMA_MASK | KG_ST_UNSUPPORTED, KG_ST_DEV_MASK | KG_ST_DEV_RSV, KG_ST_RSV_MASK. The DeviceShare
 *            code slots and KG_DIAG_FEASIBLE follow the counted word.
 * Synchronous like kg_eval_verify, with its precondition checks; the counts do not depend on index_base.
 * Counts of node shards add up: a multi-GPU caller sums the shards' rows on the host. A nonzero slot 31
 * (KG_ST_UNSUPPORTED) means the pod's diagnosis is incomplete: those pairs need the reference plugins on the host.
 * KG_INVALID_ARG: out_counts == NULL, a row >= the batch size, unknown flag bits, rows == NULL with another n_rows.
 * n_rows == 0 writes nothing; a snapshot of 0 nodes writes zeros. */
#define KG_DIAG_SLOTS 64
#define KG_DIAG_DEV_CODE0 32   /* slot 32 + c: nodes whose DeviceShare code is c (1..15); slot 32 stays 0 */
#define KG_DIAG_FEASIBLE 48    /* nodes whose status word is 0 */
#define KG_DIAG_FIRST_PLUGIN 0x1u
kg_status kg_eval_diagnose(kg_snap* snap, kg_pods* pods, const uint32_t* rows, uint32_t n_rows, uint32_t flags,
                           uint32_t* out_counts /* n_rows * KG_DIAG_SLOTS */);
/* Feasible-node bitmaps: per requested pod, which nodes of this snapshot pass Filter (one bit per pair instead of
 * kg_eval_verify's matrix). A framework-mode plugin returns row 0 as PreFilterResult{NodeNames}, serves Filter from
 * it and hands the feasible nodes to the Score plugins that stay on the host.
 *   out_bits[t * W + w], W = (n_nodes + 31) / 32, w < W: bit (i & 31) of word (i >> 5) is set iff
 *            (status word of pair (rows[t], node at snapshot position i) & fail_mask) == 0. The status word is the
 *            one kg_eval_verify reports for the pair: a batch with candidate node sets includes KG_ST_NODE_EXCLUDED,
 *            a config-5 snapshot includes the ElasticQuota gate's KG_ST_QUOTA on every node of a rejected pod. Bits
 *            at or above n_nodes in the last word are 0.
 *   fail_mask  0xFFFFFFFF: the feasible set. KG_ST_UNRESOLVABLE_MASK: the nodes where preemption might help (upstream's
 *            nodesWherePreemptionMightHelp drops the UnschedulableAndUnresolvable ones). KG_ST_UNSUPPORTED: the
 *            complement of the pairs that need the host path. 0: every node bit set.
 *   rows     as kg_eval_diagnose: batch indices, repeats and any order allowed; NULL: every pod (n_rows must equal the
 *            batch size).
 *   out_count (may be NULL): [n_rows] population count of each row.
 * The format is kg_node_sets.bits': a row can be handed back to kg_pods_set_node_sets, and the rows of node shards
 * concatenate by words when the shard sizes are multiples of 32 (else the caller shifts); each shard's call returns
 * its own nodes. index_base is not added.
 * Synchronous like kg_eval_diagnose, with its precondition checks in its order (KG_UNSUPPORTED for a batch with
 * candidate node sets on a snapshot with config-5 tables). It changes no state of the snapshot, the batch's keys or
 * kg_result_status. KG_INVALID_ARG: out_bits == NULL with n_rows > 0, a row >= the batch size, rows == NULL with
 * another n_rows. n_rows == 0 writes nothing; a snapshot of 0 nodes writes nothing to out_bits (0 words per row) and
 * zeros to out_count. The symbol is new within ABI 14: a binding resolves it at load time. */
kg_status kg_eval_feasible(kg_snap* snap, kg_pods* pods, const uint32_t* rows, uint32_t n_rows, uint32_t fail_mask,
                           uint32_t* out_bits /* n_rows * ((n_nodes + 31) / 32) */, uint32_t* out_count /* n_rows */);
/* Node offer slots of a gang: per node of this snapshot, how many of the job's pods fit when they are added to the
 * node one after another (calculateNodeOfferSlot, coscheduling/core/network_topology_solver.go:113-158), the first and
 * only expensive step of the network-topology planner (PlacePods, :53-111): the caller sums the counts up its topology
 * tree and deals the pods out on the host. Per node, independently of every other node:
 *     slot = 0; for t in 0..n_rows-1: Filter(pod rows[t], node with the first t pods added) fails ? stop : add, slot++
 * "add" is NodeInfo.AddPodInfo: the node's requested cpu / memory / ephemeral-storage / scalars, its non-zero requested
 * cpu / memory and its pod count grow by the pod's (the req_*, sc_req*, nz_* and num_pods columns). The LoadAware
 * bases, NUMA zone usage, cpusets and GPU minors stay the snapshot's: LoadAware has no AddPod hook, NodeNUMAResource's
 * and DeviceShare's return early for a pod that holds no allocation on the node. This is not the Reserve of kg_assume
 * / kg_replay, and not kg_eval_feasible's evaluation of every pod on the snapshot as it stands.
 *   rows     batch indices of the job's pods in planner order (extension.SortPodsByIndex); repeats allowed (a gang of
 *            identical pods may be uploaded once); NULL: every pod in batch order (n_rows must equal the batch size).
 *   out_slots[i], i the node's snapshot position (index_base is not added): the number of leading pods of rows that
 *            pass, 0..n_rows.
 *   out_status[i] (may be NULL): 0 when all n_rows pods passed, else the status word of the pair (rows[out_slots[i]],
 *            node i) on the node with the first out_slots[i] pods added: bit for bit the word kg_eval_verify reports
 *            on a snapshot whose columns above were raised by those pods, every failing plugin's bits. A node that
 *            stops on a word with KG_ST_UNSUPPORTED has a lower-bound count: the caller runs the reference loop there.
 * Candidate node sets of the batch are honoured, as every Filter of the host's runs in the reference's loop: a pod
 * whose set excludes the node stops the node with its usual word | KG_ST_NODE_EXCLUDED. Host score terms are ignored
 * (Filter only). Per-node results do not depend on other nodes: the outputs of node shards concatenate.
 * Synchronous like kg_eval_diagnose, with its precondition checks in its order. It changes no state of the snapshot
 * (nor its generation), the batch's keys or kg_result_status. KG_INVALID_ARG: out_slots == NULL with n_nodes > 0, a row
 * >= the batch size, rows == NULL with another n_rows, candidate node sets over another node count. n_rows == 0 writes
 * zeros to both outputs; a snapshot of 0 nodes writes nothing. KG_UNSUPPORTED: a snapshot with config-5 tables
 * (KG_PLUGIN_EXT): Reservation's AddPod (reservation/plugin.go:254-284) moves state its Filter reads, which the
 * device does not follow. The symbol is new within ABI 14: a binding resolves it at load time. */
kg_status kg_eval_offer_slots(kg_snap* snap, kg_pods* pods, const uint32_t* rows, uint32_t n_rows,
                              uint32_t* out_slots /* n_nodes */, uint32_t* out_status /* n_nodes, may be NULL */);
/* ---- Preemption dry run (PostFilter) -------------------------------------------------------------------------------
 * Resident pods of a snapshot: which pods run on each node, the table kg_eval_preempt removes victims from. One entry
 * per running pod; the columns are what SelectVictimsOnNode reads of it. */
#define KG_RES_MAX_PER_NODE 256   /* resident entries per node the device follows */
#define KG_RES_PDBS 2             /* PodDisruptionBudgets one entry can name */
#define KG_RES_NON_PREEMPTIBLE 0x1u /* extension.IsPodNonPreemptible / !IsPodPreemptible */
#define KG_RES_NUMA_ALLOC 0x2u      /* the pod holds a cpuset or NUMA-zone allocation on the node
                                       (nodenumaresource/preempt.go:227-237 getPodAllocated non-empty) */
#define KG_RES_PDB_OVERFLOW 0x4u    /* the pod matches more than KG_RES_PDBS budgets */
typedef struct kg_resident_columns {
    const uint32_t* node;        /* snapshot position (index_base not added) */
    const int32_t*  priority;    /* corev1helpers.PodPriority */
    const int64_t*  start_time;  /* GetPodStartTime, unix seconds */
    const int32_t*  group;       /* preemption group (the pod's quota name as an id), -1 = none */
    const uint32_t* flags;       /* KG_RES_* */
    const int32_t*  pdb[KG_RES_PDBS]; /* budget ids this pod counts against, -1 = unused. The host leaves out
                                         budgets whose DisruptedPods hold the pod (preempt.go:248-252) */
    const int64_t *req_cpu, *req_mem, *req_eph, *sc_req[KG_NSCALAR], *nz_cpu, *nz_mem; /* what NodeInfo.RemovePod subtracts */
} kg_resident_columns;
/* kg_snapshot_upload_residents replaces the whole table by the n rows of cols; kg_snapshot_update_residents replaces
 * the lists of the n_nodes listed nodes (each at most once) by the n rows of cols, which name only those nodes (a
 * listed node without a row ends up empty), and keeps every other list. Both copy; both bump the generation.
 * Order: the library orders each node's entries by util.MoreImportantPod: higher priority first, then earlier start
 * time; ties keep the order of the rows (of the call that supplied the list). Upstream's sort.Slice is not stable
 * there: parity unpinned on ties. A victim's "position" in every output of kg_eval_preempt is its index in that
 * ordered list; kg_snapshot_read_residents maps positions back to rows.
 * The table is kept per snapshot position, so kg_snapshot_update_rows moving records does not disturb it.
 * kg_snapshot_upload drops it. kg_assume*, kg_replay, kg_reserve and kg_batch_schedule do not touch it: the caller
 * replaces a node's list after a bind. An update sends the new lists of its nodes alone (they are appended behind the
 * table on the device; when that space is used up, one update lays the whole table out again).
 * A node with more than KG_RES_MAX_PER_NODE entries is accepted and flagged: kg_eval_preempt reports
 * KG_PREEMPT_UNSUPPORTED for it.
 * KG_INVALID_ARG: a node >= n_nodes, a NULL column with n > 0, a pdb id < -1, (update) a row naming a node that is not
 * listed, a node listed twice, no table uploaded yet. Nothing is changed then, nor by a call that fails on the device
 * (KG_OOM, KG_DEVICE_ERROR): the table of before stays in place. */
kg_status kg_snapshot_upload_residents(kg_snap* snap, const kg_resident_columns* cols, uint32_t n);
kg_status kg_snapshot_update_residents(kg_snap* snap, const uint32_t* nodes, uint32_t n_nodes,
                                       const kg_resident_columns* cols, uint32_t n);
/* The table as the library ordered it: out_count[i] = entries of the node at snapshot position i (all of them, also
 * beyond KG_RES_MAX_PER_NODE); out_row (may be NULL), node after node in position order, each node's entries in list
 * order: the row of the upload / update call that supplied the entry. Sum of out_count entries. KG_INVALID_ARG
 * without a table. */
kg_status kg_snapshot_read_residents(kg_snap* snap, uint32_t* out_count /* n_nodes */, uint32_t* out_row);

/* SelectVictimsOnNode (elasticquota/preempt.go:111-217, reservation/preemption.go:123-219) of each preemptor on
 * every node of this snapshot: the 1 + V Filter runs per node of the PostFilter dry run (preemption.Evaluator.Preempt,
 * elasticquota/plugin.go:608-619, reservation/preemption.go:102-116). Each row is one preemptor, evaluated on the
 * snapshot as it stands, independently of the other rows. Per (preemptor, node), independently of every other node:
 *  1. Potential victims: the node's entries with priority < row_priority[t]; with KG_PREEMPT_SKIP_NON_PREEMPTIBLE
 *     without those flagged KG_RES_NON_PREEMPTIBLE; with KG_PREEMPT_SAME_GROUP only those whose group equals
 *     row_group[t] (NULL: -1). None: KG_PREEMPT_NO_VICTIMS.
 *  2. All of them are removed: the node's requested cpu / memory / ephemeral-storage / scalars, its non-zero requested
 *     cpu / memory and its pod count drop by the entries' columns (NodeInfo.RemovePod; plain int64 subtraction). The
 *     LoadAware bases, NUMA zone usage, cpusets and GPU minors stay the snapshot's: LoadAware has no AddPod / RemovePod
 *     hook. The Filter word of the pair on that node is kg_eval_verify's, bit for bit, on a snapshot whose columns were
 *     lowered so. Non-zero: KG_PREEMPT_NO_FIT with that word.
 *  3. PDB split (filterPodsWithPDBViolation, preempt.go:224-269): the potential victims in list order, a fresh copy of
 *     pdb_allowed per node; each budget an entry names is decremented, and the entry is violating when any of its
 *     budgets went below 0. The order inside both groups is kept.
 *  4. Reprieve: the violating group first, then the other, each from the most important entry: the entry is added
 *     back and the word taken; 0: it stays; non-zero: it is removed again and is a victim (n_violating counts those of
 *     the first group).
 *  5. KG_PREEMPT_UNSUPPORTED, with n_victims = 0 (the host runs the reference on that node), when the node's list
 *     overflowed, a potential victim has KG_RES_PDB_OVERFLOW, a potential victim has KG_RES_NUMA_ALLOC while
 *     KG_PLUGIN_NUMA is on and the preemptor is not KG_POD_NUMA_SKIP (NodeNUMAResource's RemovePod then feeds a
 *     preemptible state its Filter reads, nodenumaresource/preempt.go:165-217, which the device does not follow), or
 *     any word taken on the node carries KG_ST_UNSUPPORTED.
 * A node outside the preemptor's candidate node set (kg_pods_set_node_sets) is KG_PREEMPT_EXCLUDED: nothing is
 * evaluated there. Precedence: EXCLUDED, the overflowed list (UNSUPPORTED), NO_VICTIMS, the victims' flags
 * (UNSUPPORTED), the word after the removal (UNSUPPORTED / NO_FIT), the reprieve's words (UNSUPPORTED), CANDIDATE.
 * Host score terms are ignored (Filter only). Nominated pods are not added (out of scope). */
#define KG_PREEMPT_SKIP_NON_PREEMPTIBLE 0x1u /* reservation/preemption.go:154, elasticquota canPreempt :290 */
#define KG_PREEMPT_SAME_GROUP 0x2u           /* canPreempt :309: victim.group == preemptor's group */
typedef struct kg_preempt_node {   /* 32 bytes */
    uint32_t status;       /* KG_ST_* word, see result */
    uint8_t  result;       /* KG_PREEMPT_* */
    uint8_t  pad_;
    uint16_t n_victims;
    uint16_t n_violating;  /* numViolatingVictim */
    uint16_t n_potential;  /* potential victims (0 for EXCLUDED and for an overflowed list) */
    int32_t  top_priority; /* highest priority among the victims */
    int64_t  sum_priority; /* plain sum of the victims' priorities */
    int64_t  top_start;    /* earliest start_time among the victims of top_priority */
} kg_preempt_node;
/* Every field but status, result and n_potential is 0 unless result is KG_PREEMPT_CANDIDATE with victims. */
#define KG_PREEMPT_CANDIDATE 0u   /* Success: the victims are valid (n_victims may be 0: the pod fits as it is); status 0 */
#define KG_PREEMPT_NO_VICTIMS 1u  /* no potential victim on the node (UnschedulableAndUnresolvable, preempt.go:150-153); status 0 */
#define KG_PREEMPT_NO_FIT 2u      /* does not fit with every potential victim removed: status = that word */
#define KG_PREEMPT_UNSUPPORTED 3u /* the host runs the reference there: status has KG_ST_UNSUPPORTED (the word that
                                     carried it, or the bit alone) */
#define KG_PREEMPT_EXCLUDED 4u    /* outside the preemptor's candidate node set: status = KG_ST_NODE_EXCLUDED, nothing evaluated */
/*   rows     as kg_eval_diagnose: batch indices of the preemptors, repeats and any order allowed; NULL: every pod
 *            (n_rows must equal the batch size).
 *   row_priority[t]  the preemptor's priority (the pod columns carry none).
 *   row_group[t]     its preemption group, NULL: -1 for all.
 *   pdb_allowed[b], b < n_pdbs: PodDisruptionBudget.Status.DisruptionsAllowed of budget id b. Every pdb id of the
 *            resident table must be < n_pdbs.
 *   out[t * n_nodes + i], i the node's snapshot position (index_base is not added).
 *   out_victims (may be NULL): [n_rows][n_nodes][KG_RES_MAX_PER_NODE / 32]; bit (k & 31) of word (k >> 5) is set iff
 *            position k of the node's list is a victim; all 0 unless result is KG_PREEMPT_CANDIDATE.
 * Per-node results do not depend on other nodes: the outputs of node shards concatenate. Synchronous like
 * kg_eval_diagnose, with its precondition checks in its order. It changes no state of the snapshot (nor its
 * generation), the batch's keys or kg_result_status. Every out entry is written. KG_INVALID_ARG: no resident table
 * uploaded, out == NULL or row_priority == NULL with n_rows > 0 and n_nodes > 0, unknown flags, a row >= the batch
 * size, rows == NULL with another n_rows, pdb_allowed == NULL with n_pdbs > 0, a pdb id of the table >= n_pdbs,
 * candidate node sets over another node count. n_rows == 0 writes nothing; a snapshot of 0 nodes writes nothing.
 * KG_UNSUPPORTED: a snapshot with config-5 tables (KG_PLUGIN_EXT): ElasticQuota's AddPod / RemovePod move
 * postFilterState.used, and Reservation's and DeviceShare's hooks move state their Filters read, which the device does
 * not follow. The symbols of this section are new within ABI 14: a binding resolves them at load time. */
kg_status kg_eval_preempt(kg_snap* snap, kg_pods* pods, const uint32_t* rows, uint32_t n_rows,
                          const int32_t* row_priority /* n_rows */, const int32_t* row_group /* n_rows or NULL */,
                          const int32_t* pdb_allowed, uint32_t n_pdbs, uint32_t flags,
                          kg_preempt_node* out /* n_rows * n_nodes */,
                          uint32_t* out_victims /* n_rows * n_nodes * (KG_RES_MAX_PER_NODE / 32), may be NULL */);
/* Sequential scheduling of pods[0..n) one at a time with Assume applied on the device between pods
 * (the reference's one-pod-per-cycle semantics). out_node[i] = global node index or -1 (no feasible node,
 * or the selected node's Reserve failed: KG_ST_NUMA_INSUF_* in out_reason).
 * out_reason (may be NULL): per pod, the OR of the KG_ST_* filter status bits over every node of the
 * snapshot as it stood in that pod's cycle (0 when every node passed) — the per-plugin reasons the
 * caller turns into the FitError diagnosis of an unschedulable pod (load_aware.go:48-51,
 * nodenumaresource/plugin.go:54-63).
 * With reservation views (KG_PLUGIN_RSV) each placement runs Reservation.Reserve on the device
 * (reservation/plugin.go:1295-1408): the pod joins its nominated reservation (Allocated += Mask(requests,
 * ResourceNames), one more assigned pod, every copy of it sharing kg_rsv_info.rid) and the node's views change as the
 * next cycle's restore would give them (transformer.go:740-935); the Reservation score (nominated reservation's
 * score, reservation order) is normalised per pod like in kg_eval_select. KG_UNSUPPORTED while a reservation holds
 * GPUs (its DeviceShare restore tables follow the reserve pods' allocations). */
kg_status kg_replay(kg_snap* snap, kg_pods* pods, int32_t* out_node, int64_t* out_total, uint32_t* out_reason);
/* Reserve/Unreserve of pod `pod` (batch index) on local node `node`. KG_RESERVE_FAILED: the NodeNUMAResource
 * Reserve fails on that node (BestEffort allocation), nothing applied. */
kg_status kg_assume(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node);
kg_status kg_forget(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, int32_t numa_zone);
/* kg_assume that also returns the NodeNUMAResource allocation it made: *out_zone as kg_verify_out.numa_zone,
 * out_zone_amounts[2 * KG_MAX_ZONES] = cpu (milli) per zone, then memory (bytes) per zone (zeros when no zone was
 * allocated). The reference keeps that allocation for the Unreserve (nodenumaresource/plugin.go:585-635 Reserve,
 * :700 Unreserve -> resource_manager.go:478-483 Release); kg_forget_numa takes it back, including a split over
 * several zones (zone code 0x40 | mask), which kg_forget refuses. */
kg_status kg_assume_numa(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, int32_t* out_zone,
                         int64_t* out_zone_amounts);
kg_status kg_forget_numa(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, int32_t numa_zone,
                         const int64_t* zone_amounts);
/* Reserve with every enabled plugin's state (NodeInfo, LoadAware, NUMA zone, DeviceShare minors via
 * defaultAllocateDevices order, ElasticQuota used); returns the NUMA zone and the GPU minor bitmask
 * the Unreserve needs (deviceshare/plugin.go:507-569, elasticquota/plugin.go:622-636). With reservation views
 * and no GPU-holding reservation it also runs Reservation.Reserve on the node's views (as kg_replay does); the
 * host copies are read back before the next kg_snapshot_update_views. kg_forget_ext cannot name the reservation:
 * the node's views turn stale until the caller re-uploads them (kg_snapshot_update_views). */
kg_status kg_assume_ext(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, int32_t* out_zone,
                        uint32_t* out_minors);
kg_status kg_forget_ext(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, int32_t numa_zone,
                        uint32_t minors);
/* GPU minors chosen for each pod by the last kg_replay (bitmask; 0 = none), n_pods entries. */
kg_status kg_replay_minors(kg_pods* pods, uint32_t* out);

/* What one Reserve took, as the reference keeps it for the Unreserve (CycleState and the plugins' caches): the NUMA
 * zone code and per-zone amounts (nodenumaresource/plugin.go:585-635 -> resource_manager.go Update), the cpuset CPUs
 * (NodeAllocation.addPodAllocation), the GPU minors (deviceshare/plugin.go:507-569) and the reservation the pod joined
 * (reservation/plugin.go:1295-1408 assumePods; rsv_rid = kg_rsv_info.rid on the node, -1 = none). */
typedef struct kg_reserve_record {
    int32_t numa_zone;                        /* the pair's kg_verify_out.numa_zone (-1 = none)              */
    uint32_t gpu_minors;                      /* DeviceShare minors taken (bit m = minor m)                  */
    int32_t rsv_rid;                          /* nominated reservation's rid, -1 = none                      */
    uint32_t flags;                           /* KG_RECORD_*                                                 */
    int64_t zone_amounts[2 * KG_MAX_ZONES];   /* cpu milli per zone, then memory bytes per zone              */
    uint64_t cpus[KG_MAX_CPUS / 64];          /* cpuset CPUs taken                                           */
} kg_reserve_record;
#define KG_RECORD_CPUSET 0x1u  /* the Reserve took cpuset CPUs (cpus) */
#define KG_RECORD_QUOTA 0x2u   /* the Reserve added the pod to its ElasticQuota's used */
#define KG_RECORD_RELEASED 0x4u /* kg_unreserve gave the record back: a second Unreserve of it is refused */

/* Reserve of pod `pod` on local node `node` with every enabled plugin (kg_assume / kg_assume_ext: NodeInfo,
 * LoadAware, NodeNUMAResource incl. cpusets, DeviceShare, ElasticQuota, Reservation.Reserve on the node's views),
 * filling *out with what the Unreserve needs. KG_RESERVE_FAILED: nothing applied. */
kg_status kg_reserve(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, kg_reserve_record* out);
/* Unreserve of a kg_reserve: every plugin gives back what the record says it took (load_aware.go:231-233,
 * nodenumaresource/plugin.go:700-720 -> resource_manager.go:478-483 Release incl. the cpuset CPUs and the NUMA
 * single / shared sets, deviceshare/plugin.go Unreserve, elasticquota/plugin.go:638-652, reservation/plugin.go:1409-1460
 * forgetPods: the reservation's Allocated and assigned pods, and the node's views as the next restore builds them).
 * The record is marked KG_RECORD_RELEASED on success; a record so marked is refused (KG_INVALID_ARG, nothing applied):
 * the reference's NodeAllocation.release and forgetPods do nothing for a pod they no longer hold (ABI 12). */
kg_status kg_unreserve(kg_snap* snap, kg_pods* pods, uint32_t pod, uint32_t node, kg_reserve_record* rec);
/* Copy of the snapshot's reservation views and infos as the device holds them (after Reservation.Reserve /
 * Unreserve on the device): n_views / n_infos entries as uploaded, in upload order. */
kg_status kg_snapshot_read_reservations(kg_snap* snap, kg_rsv_view* views, uint32_t n_views, kg_rsv_info* infos,
                                        uint32_t n_infos);
/* Copy of the GPU restore tables (kg_rsv_dev, n_devs as uploaded) as the device holds them: a Reserve / Unreserve into a
 * node with GPU-holding reservations rebuilds that node's tables (ABI 12). */
kg_status kg_snapshot_read_rsv_devs(kg_snap* snap, kg_rsv_dev* devs, uint32_t n_devs);

/* Device cpuset accumulator, one request per workgroup: out[4 * i] = the CPUs chosen for request i,
 * rc[i] = 0, -1 (ErrNotEnoughCPUs: fewer allocatable CPUs than needed) or -2 ("failed to allocate cpus").
 * Topologies need <= 8 NUMA nodes, <= 8 sockets and <= 8 CPUs per core (KG_UNSUPPORTED otherwise). */
kg_status kg_cpuset_take(kg_ctx* ctx, const kg_cpu_topo* topos, uint32_t n_topos, const kg_cpu_alloc* allocs,
                         uint32_t n_allocs, const kg_cpuset_request* reqs, uint32_t n, uint64_t* out, int32_t* rc);

/* ---- whole-job placement (FindOneNodePlugin slot, frameworkext/interface.go:118-127) ----------------
 * Checkpoint / rollback of everything Reserve changes (node records, NUMA zones, GPU minors, quota used):
 * a planner replays the job on the live snapshot and rolls back, so the plan costs no copy of the cluster
 * (the reference clones NodeInfos per plan, coscheduling/core/network_topology_workflow.go:98-118). One
 * checkpoint per snapshot; a new checkpoint replaces the old. Rollback fails if the snapshot was re-uploaded
 * or had rows updated since the checkpoint (its records may have moved). Both bump the generation. */
kg_status kg_snapshot_checkpoint(kg_snap* snap);
kg_status kg_snapshot_rollback(kg_snap* snap);

/* kg_batch_schedule result codes, per pod */
#define KG_BATCH_ASSUMED 0u     /* PreFilter + Filter passed on the planned node; Reserve applied          */
#define KG_BATCH_FAILED 1u      /* PreFilter / Filter failed on the planned node: status holds the bits    */
#define KG_BATCH_SIBLING 2u     /* after a failed pod of the same node (engine.go:188-192): its status     */
#define KG_BATCH_ROLLED_BACK 3u /* was assumed, undone because the job failed (CleanupAssumedPods)         */
#define KG_BATCH_NO_PLAN 4u     /* plan_node < 0: the job fails before any pod is assumed (batch_scheduler.go:96-101) */
/* Inline batch scheduling cycle for a planned job (batch/batch_scheduler.go:74-185 BatchSchedule,
 * batch/engine.go:92-294 RunSchedulingCycle): plan_node[j] = local node of pod j. Pods are grouped by
 * planned node; each group runs in batch order (the caller orders a node's pods by name, engine.go
 * :357-359): PreFilter (ElasticQuota gate on the current used) + Filter on that node, then Reserve. If every
 * pod is assumed the state stays committed and the call returns KG_OK; otherwise every assumed pod is
 * undone (result KG_BATCH_ROLLED_BACK, CleanupAssumedPods) and the call still returns KG_OK, the per-pod
 * codes telling which pod failed and why. out_zone / out_minors (may be NULL): NUMA zone and GPU minors
 * of each assumed pod. KG_UNSUPPORTED when some pair needs the host path (the state is rolled back) or
 * when reservation views are uploaded (a Reserve into a view changes its restore). */
kg_status kg_batch_schedule(kg_snap* snap, kg_pods* pods, const int32_t* plan_node, uint32_t* out_result,
                            uint32_t* out_status, int32_t* out_zone, uint32_t* out_minors);

/* Device time of the select / replay steps: one bracket per step, summed. A step of several device operations is
 * bracketed by HIP events on the launch stream. The one-launch top-1 select of one pod block times
 * itself with the device's wall clock instead (hipDeviceAttributeWallClockRate): its bracket runs from the first
 * workgroup's entry to the completion of the last result write, which leaves out the dispatch's launch ramp and
 * end-of-kernel release (a few microseconds). Each such launch fills a region of a device pool, one pair of times per
 * workgroup, which kg_profile_enable(ctx, 1) allocates on its first call (1 MiB of device memory on every context,
 * whether or not it runs such a select): that call can therefore fail with KG_OOM or KG_DEVICE_ERROR, and profiling
 * is then left off. kg_profile_read waits for the brackets still outstanding and returns KG_DEVICE_ERROR when a
 * launch left its region incomplete. */
kg_status kg_profile_enable(kg_ctx* ctx, int enable);
kg_status kg_profile_read(kg_ctx* ctx, double* total_ms, uint64_t* launches, int reset);

/* Multi-GPU node sharding over RCCL (one process per GPU). */
kg_status kg_shard_unique_id(uint8_t out[128]);
kg_status kg_shard_init(kg_ctx* ctx, const uint8_t id[128], int rank, int world);
/* Local select of the per-pod top k (1 <= k <= 4; k = 3 mirrors upstream
 * numberOfHighestScoredNodesToReport) + RCCL all-gather of the P x k per-shard keys + the same global
 * selectHost on every rank. out_keys (host, n_pods * k entries, descending per pod) may be NULL to leave
 * the result on the device (kg_result_keys reads it). */
kg_status kg_shard_select(kg_snap* snap, kg_pods* pods, uint32_t k, uint64_t* out_keys);

/* Host-only helpers (no device needed). */
/* Packed selection key: (total << 32) | (0xFFFFFFFF - node); max key = highest total, lowest index. */
uint64_t kg_make_key(int64_t total, uint32_t node);
int32_t kg_key_node(uint64_t key);    /* -1 for key 0 */
int64_t kg_key_total(uint64_t key);   /* -1 for key 0 */
/* Global selectHost over gathered per-shard keys: keys[shard][pod][k] -> out[pod][k]. */
kg_status kg_merge_keys(const uint64_t* keys, uint32_t n_shards, uint32_t n_pods, uint32_t k, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* KOORDGPU_H */
